// The C ABI: `align bucket` on records (include/sedef_hip.h states the contract; bucket_merge.hip holds the kernels and the
// three equivalences the device forms rely on) -- the `_host` form, which IS the reference's sweep on integer records, and the
// two device forms over one chain of launches.  The checks: sdf_entry.h (check_bucket_scalars, check_bucket).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <map>
#include <numeric>

#include "sdf_entry.h"

using namespace sdf;

namespace {
int bit_length(size_t x) {
  int b = 0;
  while (x >> b) ++b;
  return b;
}

// The launches of a call on `st`, nothing read back: d_n_out[0] = records in d_out, d_n_out[1] = records dropped.
int bucket_launch(sdf_ctx *ctx, const sdf_seed_hit *d_hits, size_t n_, const int32_t *d_chr_group, size_t n_chr, const int32_t *d_pair_order,
                  size_t n_groups, const sdf_bucket_params &P, sdf_bucket_hit *d_out, unsigned long long *d_n_out, hipStream_t st) {
  const int n = (int)n_;
  const size_t np = n_ + 1;
  // the workspace, in pieces of whole 256 bytes
  size_t at = 0;
  const auto piece = [&](size_t bytes) {
    const size_t off = at;
    at += (bytes + 255) & ~(size_t)255;
    return off;
  };
  const size_t o_recs = piece(n_ * sizeof(BucketRec)), o_sorted = piece(n_ * sizeof(BucketRec)), o_key_a = piece(n_ * 8), o_key_b = piece(n_ * 8),
               o_key_h = piece(n_ * 8), o_scan = piece(n_ * sizeof(BucketSeg)), o_val_a = piece(n_ * 4), o_val_b = piece(n_ * 4),
               o_new_run = piece(np * 4), o_run_of = piece(np * 4), o_run_start = piece(np * 4), o_box = piece(n_ * sizeof(BucketBox)),
               o_live = piece(n_ * 4);
  SDF_HIP(ctx->bk_ws.reserve(at));
  char *ws = (char *)ctx->bk_ws.p;
  BucketRec *recs = (BucketRec *)(ws + o_recs), *sorted = (BucketRec *)(ws + o_sorted);
  unsigned long long *key_a = (unsigned long long *)(ws + o_key_a), *key_b = (unsigned long long *)(ws + o_key_b),
                     *key_h = (unsigned long long *)(ws + o_key_h);
  BucketSeg *seg = (BucketSeg *)key_h, *scan = (BucketSeg *)(ws + o_scan);  // (key_hi as prepared is spent when the scan's items are made)
  uint32_t *val_a = (uint32_t *)(ws + o_val_a), *val_b = (uint32_t *)(ws + o_val_b), *new_run = (uint32_t *)(ws + o_new_run),
           *run_of = (uint32_t *)(ws + o_run_of), *run_start = (uint32_t *)(ws + o_run_start), *live = (uint32_t *)(ws + o_live);
  BucketBox *box = (BucketBox *)(ws + o_box);
  // (the class sort: keys and places in the first key buffer, sorted into the third; both are spent by then)
  uint32_t *cls_key = (uint32_t *)key_a, *cls_place = cls_key + n_, *cls_key2 = (uint32_t *)key_h, *cls_place2 = cls_key2 + n_;
  // the bits in use: q_start << 32 | r_start of coordinates below 2^31; pair : rc : q_chr : r_chr; run << 32 | r_end, a dead slot
  // all ones; a class or kBucketDeadClass
  const int lo_bits = 63, hi_bits = 39 + bit_length(n_groups * n_groups - 1), flush_bits = 32 + bit_length(n_), cls_bits = 23;
  size_t t_sort = 0, t_cls = 0, t_scan = 0, t_sum = 0;
  SDF_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, t_sort, key_a, key_b, val_a, val_b, n, 0, 64, st));
  SDF_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, t_cls, cls_key, cls_key2, cls_place, cls_place2, n, 0, cls_bits, st));
  SDF_HIP(hipcub::DeviceScan::InclusiveScan(nullptr, t_scan, seg, scan, BucketSegMax(), n, st));
  SDF_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, t_sum, new_run, run_of, (int)np, st));
  const size_t tmp = std::max({t_sort, t_cls, t_scan, t_sum}) + 256;
  SDF_HIP(ctx->bk_tmp.reserve(tmp));
  size_t tb = tmp;
  const dim3 block(256), grid((unsigned)(np + 255) / 256);  // (n + 1 lanes and more)
  SDF_HIP(hipMemsetAsync(d_n_out, 0, 2 * sizeof(unsigned long long), st));
  hipLaunchKernelGGL(bucket_prepare_kernel, grid, block, 0, st, d_hits, n, d_chr_group, (int)n_chr, d_pair_order, (int)n_groups, P.extend_ratio,
                     P.max_extend, P.merge_dist, recs, key_a, key_h, val_a, d_n_out);
  SDF_HIP(hipcub::DeviceRadixSort::SortPairs(ctx->bk_tmp.p, tb = tmp, key_a, key_b, val_a, val_b, n, 0, lo_bits, st));
  hipLaunchKernelGGL(bucket_key_gather_kernel, grid, block, 0, st, key_h, val_b, n, key_a);
  SDF_HIP(hipcub::DeviceRadixSort::SortPairs(ctx->bk_tmp.p, tb = tmp, key_a, key_b, val_b, val_a, n, 0, hi_bits, st));
  hipLaunchKernelGGL(bucket_runs_kernel, grid, block, 0, st, recs, val_a, key_b, n, sorted, seg);
  SDF_HIP(hipcub::DeviceScan::InclusiveScan(ctx->bk_tmp.p, tb = tmp, seg, scan, BucketSegMax(), n, st));
  hipLaunchKernelGGL(bucket_new_run_kernel, grid, block, 0, st, sorted, scan, n, P.merge_dist, new_run, box, live);
  SDF_HIP(hipcub::DeviceScan::ExclusiveSum(ctx->bk_tmp.p, tb = tmp, new_run, run_of, (int)np, st));
  hipLaunchKernelGGL(bucket_run_starts_kernel, grid, block, 0, st, new_run, run_of, n, run_start);
  // (a wavefront looks at 64 runs at a time and sweeps those of two or more slots: enough wavefronts for the device, no more)
  const unsigned sweep_blocks = (unsigned)std::min<size_t>((n_ + 255) / 256, 4096);
  hipLaunchKernelGGL(bucket_sweep_kernel, dim3(sweep_blocks), block, 0, st, box, live, run_start, run_of + n_, P.merge_dist);
  hipLaunchKernelGGL(bucket_flush_keys_kernel, grid, block, 0, st, box, live, new_run, run_of, n, key_a, val_a);
  SDF_HIP(hipcub::DeviceRadixSort::SortPairs(ctx->bk_tmp.p, tb = tmp, key_a, key_b, val_a, val_b, n, 0, flush_bits, st));
  hipLaunchKernelGGL(bucket_class_kernel, grid, block, 0, st, key_b, val_b, sorted, box, n, d_out, cls_key, cls_place, d_n_out);
  SDF_HIP(hipcub::DeviceRadixSort::SortPairs(ctx->bk_tmp.p, tb = tmp, cls_key, cls_key2, cls_place, cls_place2, n, 0, cls_bits, st));
  hipLaunchKernelGGL(bucket_deal_kernel, grid, block, 0, st, cls_key2, cls_place2, n, P.nbins, d_out);
  SDF_HIP(hipGetLastError());
  ctx->launches += 9;
  return SDF_OK;
}
}  // namespace

extern "C" int sdf_bucket_merge_device(sdf_ctx *ctx, const sdf_seed_hit *d_hits, size_t n, const int32_t *d_chr_group, size_t n_chr,
                                       const int32_t *d_group_pair_order, size_t n_groups, const sdf_bucket_params *params,
                                       sdf_bucket_hit *d_out, size_t out_cap, uint64_t *d_n_out) {
  if (!ctx) return SDF_ERR_INVALID;
  ctx->err.clear();
  const char *why = "";
  if (int rc = check_bucket_scalars(d_hits, n, d_chr_group, n_chr, d_group_pair_order, n_groups, params, d_out, out_cap, d_n_out, &why))
    return refuse(ctx, rc, std::string("sdf_bucket_merge_device: ") + why);
  SDF_HIP(hipSetDevice(ctx->device));
  if (n == 0) {
    SDF_HIP(hipMemsetAsync(d_n_out, 0, 2 * sizeof(uint64_t), ctx->stream));
    return SDF_OK;
  }
  return bucket_launch(ctx, d_hits, n, d_chr_group, n_chr, d_group_pair_order, n_groups, *params, d_out, (unsigned long long *)d_n_out, ctx->stream);
}

extern "C" int sdf_bucket_merge(sdf_ctx *ctx, const sdf_seed_hit *hits, size_t n, const int32_t *chr_group, size_t n_chr,
                                const int32_t *group_pair_order, size_t n_groups, const sdf_bucket_params *params, sdf_bucket_hit *out,
                                size_t out_cap, size_t *n_out) {
  if (!ctx) return SDF_ERR_INVALID;
  ctx->err.clear();
  std::string why;
  {
    std::vector<BucketRec> recs;  // (the device prepares its own)
    if (int rc = check_bucket(hits, n, chr_group, n_chr, group_pair_order, n_groups, params, out, out_cap, n_out, &recs, &why))
      return refuse(ctx, rc, "sdf_bucket_merge: " + why);
  }
  *n_out = 0;
  if (n == 0) return SDF_OK;
  SDF_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  SDF_HIP(ctx->bk_out.reserve(n * sizeof(sdf_bucket_hit) + 2 * sizeof(uint64_t)));
  if (int rc = upload_all(ctx, st, {{ctx->bk_in, hits, n * sizeof(sdf_seed_hit)},
                                    {ctx->bk_chr, chr_group, n_chr * sizeof(int32_t)},
                                    {ctx->bk_pairs, group_pair_order, n_groups * n_groups * sizeof(int32_t)}}))
    return rc;
  unsigned long long *d_n_out = (unsigned long long *)ctx->bk_out.p;
  sdf_bucket_hit *d_out = (sdf_bucket_hit *)(d_n_out + 2);
  if (int rc = bucket_launch(ctx, (const sdf_seed_hit *)ctx->bk_in.p, n, (const int32_t *)ctx->bk_chr.p, n_chr, (const int32_t *)ctx->bk_pairs.p,
                             n_groups, *params, d_out, d_n_out, st))
    return rc;
  unsigned long long counts[2] = {0, 0};
  SDF_HIP(hipMemcpyAsync(counts, d_n_out, sizeof counts, hipMemcpyDeviceToHost, st));
  SDF_HIP(hipStreamSynchronize(st));
  if (counts[1] != 0 || counts[0] > n)  // (the host's check passed every record: the two disagree)
    return refuse(ctx, SDF_ERR_INVALID, "sdf_bucket_merge: the device dropped " + std::to_string(counts[1]) + " records the host's check passed");
  if (counts[0]) SDF_HIP(hipMemcpyAsync(out, d_out, counts[0] * sizeof(sdf_bucket_hit), hipMemcpyDeviceToHost, st));
  SDF_HIP(hipStreamSynchronize(st));
  *n_out = (size_t)counts[0];
  return SDF_OK;
}

// The host form: the reference's sweep as bucket.cc states it (merge_hits), on the prepared records -- the multimap of windows
// by reference end, the lower_bound, the grow loop, `last` --, and its deal with the per-class counters.
extern "C" int sdf_bucket_merge_host(const sdf_seed_hit *hits, size_t n, const int32_t *chr_group, size_t n_chr, const int32_t *group_pair_order,
                                     size_t n_groups, const sdf_bucket_params *params, sdf_bucket_hit *out, size_t out_cap, size_t *n_out) {
  std::string why;
  std::vector<BucketRec> recs;
  if (int rc = check_bucket(hits, n, chr_group, n_chr, group_pair_order, n_groups, params, out, out_cap, n_out, &recs, &why)) return rc;
  *n_out = 0;
  if (n == 0) return SDF_OK;
  const int32_t merge_dist = params->merge_dist;
  std::vector<uint32_t> order(n);
  std::iota(order.begin(), order.end(), 0u);
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
    const uint64_t ha = bucket_key_hi(recs[a]), hb = bucket_key_hi(recs[b]);
    return ha != hb ? ha < hb : bucket_key_lo(recs[a]) < bucket_key_lo(recs[b]);
  });
  size_t m = 0;
  std::multimap<int32_t, BucketBox> windows;  // by reference end
  const BucketRec *run = nullptr;              // (names and strand of the run's hits)
  const auto flush = [&] {
    for (auto &w : windows)
      out[m++] = sdf_bucket_hit{run->q_chr, w.second.q_start, w.second.q_end, run->r_chr, w.second.r_start, w.second.r_end, run->flags & SDF_SEED_RC, 0};
    windows.clear();
  };
  int32_t last_q_end = 0;
  for (size_t k = 0; k < n; k++) {
    const BucketRec &r = recs[order[k]];
    if (r.flags & kBucketSelf) continue;
    BucketBox h{r.q_start, r.q_end, r.r_start, r.r_end};
    const bool new_run = !run || last_q_end + merge_dist < h.q_start || bucket_key_hi(*run) != bucket_key_hi(r);
    if (new_run) {
      flush();
    } else {
      for (bool grew = true; grew;) {
        grew = false;
        for (auto w = windows.lower_bound(h.r_start - merge_dist); w != windows.end();) {
          if (bucket_apart(w->second, h, merge_dist)) {
            ++w;
            continue;
          }
          h.q_start = std::min(h.q_start, w->second.q_start);
          h.q_end = std::max(h.q_end, w->second.q_end);
          h.r_start = std::min(h.r_start, w->second.r_start);
          h.r_end = std::max(h.r_end, w->second.r_end);
          w = windows.erase(w);
          grew = true;
        }
      }
    }
    windows.emplace(h.r_end, h);
    last_q_end = new_run ? h.q_end : std::max(h.q_end, last_q_end);
    run = &r;
  }
  if (run) flush();
  // the deal (src/align_main.cc:147-175): every class round the buckets on its own, from where the class below stopped
  int32_t top = 0;
  for (size_t j = 0; j < m; j++) top = std::max(top, bucket_class(BucketBox{out[j].q_start, out[j].q_end, out[j].r_start, out[j].r_end}));
  std::vector<int64_t> per_class((size_t)top + 1, 0), next_bucket((size_t)top + 1, 0);
  for (size_t j = 0; j < m; j++) per_class[(size_t)bucket_class(BucketBox{out[j].q_start, out[j].q_end, out[j].r_start, out[j].r_end})]++;
  for (size_t c = 1; c <= (size_t)top; c++) next_bucket[c] = (next_bucket[c - 1] + per_class[c - 1]) % params->nbins;
  for (size_t j = 0; j < m; j++) {
    int64_t &turn = next_bucket[(size_t)bucket_class(BucketBox{out[j].q_start, out[j].q_end, out[j].r_start, out[j].r_end})];
    out[j].bucket = (int32_t)turn;
    turn = (turn + 1) % params->nbins;
  }
  *n_out = m;
  return SDF_OK;
}
