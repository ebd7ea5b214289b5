// The C ABI: pair recall (include/sedef_hip.h states the contract; pair_recall.hip holds the kernels; the rule is
// sdf_kernels.h's recall_* functions) -- the `_host` form, the form over host arrays and the device form over one chain of
// launches.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <memory>

#include "sdf_entry.h"

using namespace sdf;

namespace {
constexpr size_t kRecallMaxGold = (size_t)1 << 30, kRecallMaxFound = (size_t)1 << 29;

// what every form asks of its scalars, in order; the pointers are the caller's arrays wherever they lie
int check_recall_scalars(const void *gold, size_t n_gold, const void *found, size_t n_found, uint32_t flags, const void *out, const char **why) {
  if (flags & ~SDF_RECALL_IGNORE_STRAND) return *why = "unknown call flag", SDF_ERR_UNSUPPORTED;
  if (n_gold > kRecallMaxGold || n_found > kRecallMaxFound) return *why = "more than 2^30 gold or 2^29 found records in one call", SDF_ERR_UNSUPPORTED;
  if ((n_gold && (!gold || !out)) || (n_found && !found)) return *why = "invalid arguments", SDF_ERR_INVALID;
  return SDF_OK;
}
// ... and, where the arrays are the host's, of every record
int check_recall(const sdf_pair_rec *gold, size_t n_gold, const sdf_pair_rec *found, size_t n_found, uint32_t flags, const void *out,
                 std::string *why) {
  const char *w = "";
  if (int rc = check_recall_scalars(gold, n_gold, found, n_found, flags, out, &w)) return *why = w, rc;
  const auto bad = [&](const char *set, size_t i) {
    return *why = std::string(set) + " record " + std::to_string(i) + ": start > end, a start or a chromosome id below 0, a flags bit above 1 or reserved != 0",
           SDF_ERR_INVALID;
  };
  for (size_t i = 0; i < n_gold; i++)
    if (recall_rec_bad(gold[i])) return bad("gold", i);
  for (size_t i = 0; i < n_found; i++)
    if (recall_rec_bad(found[i])) return bad("found", i);
  return SDF_OK;
}

// The host's index of the found records: what recall_entries_kernel and the sort leave on the device.
struct RecallIndex {
  std::vector<std::pair<unsigned long long, uint32_t>> ent;  // (key, 2 * record + end) of every end with a base, ascending
  int32_t max_len = 0;
  RecallIndex(const sdf_pair_rec *found, size_t n_found) {
    ent.reserve(2 * n_found);
    for (size_t i = 0; i < n_found; i++)
      for (int e = 0; e < 2; e++) {
        const RecallEnd E = recall_end(found[i], e);
        if (E.end <= E.start) continue;
        ent.emplace_back(recall_key(E.chr, E.start), (uint32_t)(2 * i + (size_t)e));
        max_len = std::max(max_len, E.end - E.start);
      }
    std::sort(ent.begin(), ent.end());
  }
};

// the bases inside the union of clipped intervals (start << 32 | end): sorted by start, each adds what lies behind the largest
// end in front of it
int32_t recall_union_host(std::vector<unsigned long long> &iv) {
  std::sort(iv.begin(), iv.end());
  long long total = 0, reach = 0;
  for (const unsigned long long v : iv) {
    const long long start = (long long)(v >> 32), end = (long long)(v & 0xFFFFFFFFull);
    total += std::max(0ll, end - std::max(start, reach));
    reach = std::max(reach, end);
  }
  return (int32_t)total;
}

// one gold record against the index: the walk of recall_kernel without its cap
sdf_pair_recall_rec recall_one_host(const sdf_pair_rec &G, const sdf_pair_rec *found, const RecallIndex &X, bool ignore_strand,
                                    std::vector<unsigned long long> &l1, std::vector<unsigned long long> &l2) {
  sdf_pair_recall_rec R{0u, 0, 0, 0u};
  if (G.end1 <= G.start1 || G.end2 <= G.start2 || X.max_len == 0) return R;
  l1.clear(), l2.clear();
  const auto first = [&](unsigned long long key) {
    return std::lower_bound(X.ent.begin(), X.ent.end(), std::make_pair(key, (uint32_t)0));
  };
  for (auto it = first(recall_key(G.chr1, (long long)G.start1 - X.max_len + 1)), end = first(recall_key(G.chr1, G.end1)); it < end; ++it) {
    bool hit, counts;
    unsigned long long iv1, iv2;
    recall_entry(G, found[it->second >> 1], (int)(it->second & 1u), ignore_strand, &hit, &counts, &iv1, &iv2);
    if (hit) l1.push_back(iv1), l2.push_back(iv2);
    R.n_hits += counts;
  }
  if (l1.size() > (size_t)kRecallCap) R.flags |= SDF_RECALL_WIDE;
  R.cov1 = recall_union_host(l1);
  R.cov2 = recall_union_host(l2);
  return R;
}

// The launches of a call on `st`, nothing read back: d_status[0] = found records dropped, d_status[1] = gold records dropped.
int recall_launch(sdf_ctx *ctx, const sdf_pair_rec *d_gold, size_t n_gold, const sdf_pair_rec *d_found, size_t n_found, uint32_t flags,
                  sdf_pair_recall_rec *d_out, unsigned long long *d_status, hipStream_t st) {
  const size_t n_ent = 2 * n_found;
  // the workspace, in pieces of whole 256 bytes: the longest end, then the entries as made and as sorted
  size_t at = 0;
  const auto piece = [&](size_t bytes) {
    const size_t off = at;
    at += (bytes + 255) & ~(size_t)255;
    return off;
  };
  const size_t o_max = piece(sizeof(int32_t)), o_key_a = piece(n_ent * 8), o_key_b = piece(n_ent * 8), o_val_a = piece(n_ent * 4),
               o_val_b = piece(n_ent * 4);
  SDF_HIP(ctx->rc_ws.reserve(at));
  char *ws = (char *)ctx->rc_ws.p;
  int32_t *max_len = (int32_t *)(ws + o_max);
  unsigned long long *key_a = (unsigned long long *)(ws + o_key_a), *key_b = (unsigned long long *)(ws + o_key_b);
  uint32_t *val_a = (uint32_t *)(ws + o_val_a), *val_b = (uint32_t *)(ws + o_val_b);
  SDF_HIP(hipMemsetAsync(max_len, 0, sizeof(int32_t), st));  // (every call's own: nothing of the call before is read)
  SDF_HIP(hipMemsetAsync(d_status, 0, 2 * sizeof(unsigned long long), st));
  if (n_found) {
    size_t tmp = 0;
    SDF_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp, key_a, key_b, val_a, val_b, (int)n_ent, 0, 64, st));
    tmp += 256;
    SDF_HIP(ctx->rc_tmp.reserve(tmp));
    hipLaunchKernelGGL(recall_entries_kernel, dim3((unsigned)((n_found + 255) / 256)), dim3(256), 0, st, d_found, (int)n_found, key_a, val_a,
                       max_len, d_status);
    SDF_HIP(hipcub::DeviceRadixSort::SortPairs(ctx->rc_tmp.p, tmp, key_a, key_b, val_a, val_b, (int)n_ent, 0, 64, st));
    ctx->launches += 1;
  }
  hipLaunchKernelGGL(recall_kernel, dim3((unsigned)n_gold), dim3(64), 0, st, d_gold, d_found, (const unsigned long long *)key_b,
                     (const uint32_t *)val_b, (int)n_ent, (const int32_t *)max_len, flags, d_out, d_status);
  ctx->launches += 1;
  SDF_HIP(hipGetLastError());
  return SDF_OK;
}
}  // namespace

extern "C" int sdf_pair_recall_device(sdf_ctx *ctx, const sdf_pair_rec *d_gold, size_t n_gold, const sdf_pair_rec *d_found, size_t n_found,
                                      uint32_t flags, sdf_pair_recall_rec *d_out, uint64_t *d_status) {
  if (!ctx) return SDF_ERR_INVALID;
  ctx->err.clear();
  const char *why = "";
  if (int rc = check_recall_scalars(d_gold, n_gold, d_found, n_found, flags, d_out, &why))
    return refuse(ctx, rc, std::string("sdf_pair_recall_device: ") + why);
  if (!d_status) return refuse(ctx, SDF_ERR_INVALID, "sdf_pair_recall_device: invalid arguments");
  SDF_HIP(hipSetDevice(ctx->device));
  if (n_gold == 0) {
    SDF_HIP(hipMemsetAsync(d_status, 0, 2 * sizeof(uint64_t), ctx->stream));
    return SDF_OK;
  }
  return recall_launch(ctx, d_gold, n_gold, d_found, n_found, flags, d_out, (unsigned long long *)d_status, ctx->stream);
}

extern "C" int sdf_pair_recall(sdf_ctx *ctx, const sdf_pair_rec *gold, size_t n_gold, const sdf_pair_rec *found, size_t n_found, uint32_t flags,
                               sdf_pair_recall_rec *out) {
  if (!ctx) return SDF_ERR_INVALID;
  ctx->err.clear();
  std::string why;
  if (int rc = check_recall(gold, n_gold, found, n_found, flags, out, &why)) return refuse(ctx, rc, "sdf_pair_recall: " + why);
  if (n_gold == 0) return SDF_OK;
  SDF_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  for (DevBuf *b : {&ctx->rc_ws, &ctx->rc_tmp, &ctx->rc_gold, &ctx->rc_found, &ctx->rc_out}) b->new_call();
  SDF_HIP(ctx->rc_out.reserve(2 * sizeof(uint64_t) + n_gold * sizeof(sdf_pair_recall_rec)));
  if (int rc = upload_all(ctx, st, {{ctx->rc_gold, gold, n_gold * sizeof(sdf_pair_rec)}, {ctx->rc_found, found, n_found * sizeof(sdf_pair_rec)}}))
    return rc;
  unsigned long long *d_status = (unsigned long long *)ctx->rc_out.p;
  sdf_pair_recall_rec *d_out = (sdf_pair_recall_rec *)(d_status + 2);
  if (int rc = recall_launch(ctx, (const sdf_pair_rec *)ctx->rc_gold.p, n_gold, (const sdf_pair_rec *)ctx->rc_found.p, n_found, flags, d_out,
                             d_status, st))
    return rc;
  unsigned long long status[2] = {0, 0};
  SDF_HIP(hipMemcpyAsync(status, d_status, sizeof status, hipMemcpyDeviceToHost, st));
  SDF_HIP(hipMemcpyAsync(out, d_out, n_gold * sizeof(sdf_pair_recall_rec), hipMemcpyDeviceToHost, st));
  SDF_HIP(hipStreamSynchronize(st));
  if (status[0] != 0 || status[1] != 0)  // (the host's check passed every record: the two disagree)
    return refuse(ctx, SDF_ERR_INVALID, "sdf_pair_recall: the device dropped " + std::to_string(status[0]) + " found and " +
                                            std::to_string(status[1]) + " gold records the host's check passed");
  // the records whose lists LDS does not hold: the same walk on the host, without a cap
  std::unique_ptr<RecallIndex> X;
  std::vector<unsigned long long> l1, l2;
  for (size_t g = 0; g < n_gold; g++) {
    if (!(out[g].flags & SDF_RECALL_WIDE)) continue;
    if (!X) X.reset(new RecallIndex(found, n_found));
    out[g] = recall_one_host(gold[g], found, *X, (flags & SDF_RECALL_IGNORE_STRAND) != 0, l1, l2);
  }
  return SDF_OK;
}

extern "C" int sdf_pair_recall_host(const sdf_pair_rec *gold, size_t n_gold, const sdf_pair_rec *found, size_t n_found, uint32_t flags,
                                    sdf_pair_recall_rec *out) {
  std::string why;
  if (int rc = check_recall(gold, n_gold, found, n_found, flags, out, &why)) return rc;
  if (n_gold == 0) return SDF_OK;
  const RecallIndex X(found, n_found);
  std::vector<unsigned long long> l1, l2;
  for (size_t g = 0; g < n_gold; g++) out[g] = recall_one_host(gold[g], found, X, (flags & SDF_RECALL_IGNORE_STRAND) != 0, l1, l2);
  return SDF_OK;
}
