// The C ABI, seeding: anchors of pairs of ranges and their chains (anchors.hip, chain.hip).
#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>

#include "sdf_entry.h"

using namespace sdf;

// ---- seed anchors (reference: src/chain.cc:24-101) ---------------------------------------------------
static int anchors_range(sdf_ctx *ctx, const sdf_anchor_pair *pairs, const uint8_t *r_rc, size_t n, const char *d_pool, int kmer,
                         int pos_bits, sdf_anchor *out, size_t out_cap, int64_t *out_off, size_t *out_used, hipStream_t st) {
  using namespace sdf;
  Lap lap{ctx->cfg.debug_timing != 0, "[anchors_range: %s %.2f ms]\n"};  // (host milliseconds of the call's sections)
  int pair_bits = 1;
  while (((size_t)1 << pair_bits) <= n) ++pair_bits;  // (strictly more than n - 1 needs: the all-ones pair field is the invalid keys' alone)
  const int key_bits = std::min(64, pair_bits + 2 * kmer + pos_bits);  // (the sort looks at the bits in use only)
  std::vector<AnchorPairDev> hp(n);
  long long nrk = 0, nqk = 0;
  bool any_rc = false;  // (a call without a reversed reference runs the kernels without the strand test)
  for (size_t i = 0; i < n; i++) {
    AnchorPairDev &d = hp[i];
    d.q_off = pairs[i].q_off;
    d.r_off = pairs[i].r_off;
    d.qlen = pairs[i].qlen;
    d.rlen = pairs[i].rlen;
    d.same_chr = (pairs[i].same_chr ? kPairSameChr : 0) | (r_rc && r_rc[i] ? kPairRefRc : 0);
    any_rc = any_rc || (r_rc && r_rc[i]);
    d.delta = pairs[i].delta;
    d.rk_start = nrk;
    d.qk_start = nqk;
    nrk += std::max(0, d.rlen - kmer + 1);
    nqk += std::max(0, d.qlen - kmer + 1);
  }
  for (size_t i = 0; i <= n; i++) out_off[i] = 0;
  *out_used = 0;
  if (nrk == 0 || nqk == 0) return SDF_OK;
  SDF_HIP(ctx->an_pairs.reserve(n * sizeof(AnchorPairDev)));
  SDF_HIP(ctx->an_keys.reserve((size_t)nrk * 8));
  SDF_HIP(ctx->an_keys2.reserve((size_t)nrk * 8));
  SDF_HIP(ctx->an_q.reserve((size_t)nqk * 16));
  SDF_HIP(ctx->an_off.reserve((size_t)(nqk + 1) * 8));
  SDF_HIP(ctx->an_outoff.reserve((n + 1) * 8));
  AnchorPairDev *d_pairs = (AnchorPairDev *)ctx->an_pairs.p;
  unsigned long long *d_keys = (unsigned long long *)ctx->an_keys.p, *d_keys2 = (unsigned long long *)ctx->an_keys2.p;
  uint32_t *d_qlo = (uint32_t *)ctx->an_q.p, *d_qcnt = d_qlo + nqk, *d_qeff = d_qcnt + nqk, *d_qpair = d_qeff + nqk;
  unsigned long long *d_off = (unsigned long long *)ctx->an_off.p;
  lap("pair records, buffers");
  SDF_HIP(hipMemcpyAsync(d_pairs, hp.data(), n * sizeof(AnchorPairDev), hipMemcpyHostToDevice, st));
  const dim3 grid(32, (unsigned)std::min<size_t>(n, 65535), (unsigned)((n + 65534) / 65535));
  hipLaunchKernelGGL(any_rc ? ref_keys_kernel<true> : ref_keys_kernel<false>, grid, dim3(256), 0, st, d_pairs, (int)n, d_pool, kmer, pos_bits, d_keys);
  size_t tmp_bytes = 0;
  SDF_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, tmp_bytes, d_keys, d_keys2, (int)nrk, pos_bits, key_bits, st));
  size_t scan_bytes = 0;
  SDF_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, (uint32_t *)nullptr, (unsigned long long *)nullptr,
                                           (int)(nqk + 1), st));
  SDF_HIP(ctx->an_tmp.reserve(std::max(tmp_bytes, scan_bytes) + 256));
  // (the keys are written in ascending position inside each pair and the sort is stable: the position bits need no pass)
  SDF_HIP(hipcub::DeviceRadixSort::SortKeys(ctx->an_tmp.p, tmp_bytes, d_keys, d_keys2, (int)nrk, pos_bits, key_bits, st));
  hipLaunchKernelGGL(query_lookup_kernel, grid, dim3(256), 0, st, d_pairs, (int)n, d_pool, kmer, pos_bits, d_keys2, nrk, d_qlo,
                     d_qcnt, d_qeff, d_qpair);
  // exclusive scan over nqk+1 entries (the extra input element is ignored by the exclusive form)
  SDF_HIP(hipcub::DeviceScan::ExclusiveSum(ctx->an_tmp.p, scan_bytes, d_qeff, d_off, (int)(nqk + 1), st));
  unsigned long long ncand = 0;
  SDF_HIP(hipMemcpyAsync(&ncand, d_off + nqk, 8, hipMemcpyDeviceToHost, st));
  lap("keys, sort, lookup, scan enqueued");
  SDF_HIP(hipStreamSynchronize(st));
  lap("... done on the device");
  if (ncand == 0) return SDF_OK;
  if (ncand > (1ull << 30)) {
    ctx->err = "anchor candidates exceed 2^30 in one batch";
    return SDF_ERR_NOMEM;
  }
  SDF_HIP(ctx->an_flag.reserve((size_t)(ncand + 1) * 4));
  SDF_HIP(ctx->an_pos.reserve((size_t)(ncand + 1) * 8));
  SDF_HIP(ctx->an_cand.reserve((size_t)ncand * sizeof(CandOut)));
  uint32_t *d_flag = (uint32_t *)ctx->an_flag.p;
  unsigned long long *d_pos = (unsigned long long *)ctx->an_pos.p;
  CandOut *d_cand = (CandOut *)ctx->an_cand.p;
  const unsigned nb = (unsigned)((ncand + 255) / 256);
  hipLaunchKernelGGL(any_rc ? candidates_kernel<true> : candidates_kernel<false>, dim3(nb), dim3(256), 0, st, d_pairs, d_pool, kmer, d_keys2, d_qlo, d_qcnt, d_off,
                     d_qpair, nqk, (long long)ncand, d_flag, d_cand, pos_bits);
  SDF_HIP(hipMemsetAsync(d_flag + ncand, 0, 4, st));
  size_t scan2 = 0;
  SDF_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, scan2, d_flag, d_pos, (int)(ncand + 1), st));
  SDF_HIP(ctx->an_tmp.reserve(scan2 + 256));
  SDF_HIP(hipcub::DeviceScan::ExclusiveSum(ctx->an_tmp.p, scan2, d_flag, d_pos, (int)(ncand + 1), st));
  unsigned long long total = 0;
  SDF_HIP(hipMemcpyAsync(&total, d_pos + ncand, 8, hipMemcpyDeviceToHost, st));
  SDF_HIP(hipStreamSynchronize(st));
  lap("candidates + scan");
  *out_used = (size_t)total;
  long long *d_outoff = (long long *)ctx->an_outoff.p;
  hipLaunchKernelGGL(anchor_offsets_kernel, dim3((unsigned)((n + 256) / 256)), dim3(256), 0, st, d_pairs, (int)n, d_off,
                     d_pos, (long long)ncand, total, nqk, d_outoff);
  SDF_HIP(hipMemcpyAsync(out_off, d_outoff, (n + 1) * 8, hipMemcpyDeviceToHost, st));
  if (total > out_cap) {
    SDF_HIP(hipStreamSynchronize(st));
    ctx->err = "anchor output buffer too small";
    return SDF_ERR_CIGAR_OVERFLOW;
  }
  if (total) {
    const size_t bytes = (size_t)total * sizeof(sdf_anchor);
    static_assert(sizeof(CandOut) == sizeof(sdf_anchor), "the compaction writes anchors as they go out");
    const bool out_is_pinned = (const uint8_t *)out >= (const uint8_t *)ctx->host_an.p &&
                               (const uint8_t *)out + bytes <= (const uint8_t *)ctx->host_an.p + ctx->host_an.cap;
    // (sdf_anchors_batch_view: the caller reads the pinned staging itself, and the compaction kernel WRITES it there -- sixteen
    // bytes a lane, coalesced, over PCIe; an asynchronous device-to-host copy of the same 34 MB behind the kernel cost its
    // caller 7-8 ms to enqueue)
    if (!out_is_pinned) SDF_HIP(ctx->an_out.reserve((size_t)total * sizeof(CandOut)));
    hipLaunchKernelGGL(anchors_compact_kernel, dim3(nb), dim3(256), 0, st, d_flag, d_pos, d_cand, (long long)ncand,
                       out_is_pinned ? (CandOut *)out : (CandOut *)ctx->an_out.p, total);
    if (out_is_pinned) {
    } else if (bytes >= ((size_t)1 << 20) && bytes <= ctx->host_an.cap) {  // through pinned staging, copied out on a few threads
      SDF_HIP(hipMemcpyAsync(ctx->host_an.p, ctx->an_out.p, bytes, hipMemcpyDeviceToHost, st));
      SDF_HIP(hipStreamSynchronize(st));
      const int nthr = 4;
      std::vector<std::thread> thr;
      auto part = [&](int q) {
        const size_t a = bytes * (size_t)q / nthr, b = bytes * (size_t)(q + 1) / nthr;
        memcpy((uint8_t *)out + a, (const uint8_t *)ctx->host_an.p + a, b - a);
      };
      for (int q = 1; q < nthr; ++q) thr.emplace_back(part, q);
      part(0);
      for (auto &t : thr) t.join();
    } else {
      SDF_HIP(hipMemcpyAsync(out, ctx->an_out.p, bytes, hipMemcpyDeviceToHost, st));
    }
  }
  SDF_HIP(hipStreamSynchronize(st));
  lap("compaction + anchors to the host");
  SDF_HIP(hipGetLastError());
  return SDF_OK;
}

extern "C" int sdf_anchors_batch_strand(sdf_ctx *ctx, const sdf_anchor_pair *pairs, const uint8_t *r_rc, size_t n, const char *seq_pool,
                                        size_t pool_bytes, int kmer, sdf_anchor *out, size_t out_cap, int64_t *out_off,
                                        size_t *out_used) {
  if (!ctx) return SDF_ERR_INVALID;
  ctx->err.clear();
  if (out_used) *out_used = 0;
  if (!pairs || !out_off || !out_used) {
    ctx->err = "invalid arguments";
    return SDF_ERR_INVALID;
  }
  const bool resident = !seq_pool && pool_bytes;  // (the characters sdf_pool_upload left in HBM)
  if (resident && pool_bytes > ctx->pool_bytes) {
    ctx->err = "the resident pool (sdf_pool_upload) is shorter than pool_bytes";
    return SDF_ERR_INVALID;
  }
  if (kmer < 1 || kmer > 15) {  // (the reference's hash is the 2-bit code of the k-mer in 32 bits, src/chain.cc:30-35)
    ctx->err = "GPU anchors implement k-mer sizes up to 15";
    return SDF_ERR_UNSUPPORTED;
  }
  int32_t rmax = 1;
  for (size_t i = 0; i < n; i++) {
    const sdf_anchor_pair &p = pairs[i];
    if (p.qlen < 0 || p.rlen < 0) {
      ctx->err = "negative sequence length";
      return SDF_ERR_INVALID;
    }
    rmax = std::max(rmax, p.rlen);
    if (p.q_off < 0 || p.r_off < 0 || (size_t)p.q_off + p.qlen > pool_bytes || (size_t)p.r_off + p.rlen > pool_bytes) {
      ctx->err = "pair sequence range outside the pool";
      return SDF_ERR_INVALID;
    }
  }
  SDF_HIP(hipSetDevice(ctx->device));
  if (n == 0) {
    out_off[0] = 0;
    return SDF_OK;
  }
  const bool dbg_t = ctx->cfg.debug_timing != 0;
  const auto dbg0 = std::chrono::steady_clock::now();
  if (!resident) {  // (the pool stays where it is after the call: sdf_extz2_batch_pairs may name ranges of it)
    if (pool_writable(ctx) != SDF_OK) return SDF_ERR_INVALID;
    ctx->pool_bytes = 0;
    ctx->pool_epoch += 1;
    SDF_HIP(ctx->an_pool.reserve(pool_bytes + 64));
    SDF_HIP(hipMemcpyAsync(ctx->an_pool.p, seq_pool, pool_bytes, hipMemcpyHostToDevice, ctx->stream));
    ctx->pool_bytes = pool_bytes;
  }
  if (dbg_t) SDF_HIP(hipStreamSynchronize(ctx->stream));
  const auto dbg1 = std::chrono::steady_clock::now();
  // Key = pair | hash (2k bits) | position: the pairs are run in ranges that fit the bits the other two fields leave (k = 11
  // and references of up to 100 kb: 33 million pairs a range; k = 15 and 5 Mb: 2,048) -- and whose k-mers fit 32-bit indices.
  int pos_bits = 1;
  while (pos_bits < 31 && ((int64_t)1 << pos_bits) < (int64_t)rmax) ++pos_bits;
  const int pair_bits = std::min(30, 64 - 2 * kmer - pos_bits);
  const size_t range_max = ((size_t)1 << pair_bits) - 1;  // (a range's pair field never reaches all ones: anchors_range)
  int rc = SDF_OK;
  size_t used_total = 0;
  out_off[0] = 0;
  for (size_t s = 0; s < n && rc == SDF_OK;) {
    size_t e = s;
    int64_t nrk = 0, nqk = 0;
    while (e < n && e - s < range_max) {
      const int64_t a = std::max(0, pairs[e].rlen - kmer + 1), b = std::max(0, pairs[e].qlen - kmer + 1);
      if (e > s && (nrk + a > 0x7fffff00ll || nqk + b > 0x7fffff00ll)) break;
      nrk += a, nqk += b;
      ++e;
    }
    if (nrk > 0x7fffff00ll || nqk > 0x7fffff00ll) {
      ctx->err = "a pair of sequences of 2 Gb or more";
      return SDF_ERR_UNSUPPORTED;
    }
    size_t used = 0;
    const int64_t first = out_off[s];
    rc = anchors_range(ctx, pairs + s, r_rc ? r_rc + s : nullptr, e - s, (const char *)ctx->an_pool.p, kmer, pos_bits, out ? out + used_total : nullptr,
                       out_cap > used_total ? out_cap - used_total : 0, out_off + s, &used, ctx->stream);
    for (size_t i = s; i <= e; i++) out_off[i] += first;  // (the range's offsets start at 0)
    if (rc == SDF_ERR_CIGAR_OVERFLOW) {  // the caller wants the size needed: count the remaining ranges too
      size_t more = 0;
      for (size_t s2 = e; s2 < n;) {
        size_t e2 = std::min(n, s2 + range_max), u2 = 0;
        std::vector<int64_t> tmp_off(e2 - s2 + 1);
        (void)anchors_range(ctx, pairs + s2, r_rc ? r_rc + s2 : nullptr, e2 - s2, (const char *)ctx->an_pool.p, kmer, pos_bits, nullptr, 0, tmp_off.data(), &u2,
                            ctx->stream);
        more += u2;
        s2 = e2;
      }
      used_total += used + more;
      break;
    }
    used_total += used;
    s = e;
  }
  *out_used = used_total;
  if (dbg_t)
    fprintf(stderr, "[sdf_anchors_batch n=%zu pool=%zu anchors=%zu] upload %.1f ms, rest %.1f ms\n", n, pool_bytes, *out_used,
            ms_between(dbg0, dbg1), ms_since(dbg1));
  return rc;
}

extern "C" int sdf_anchors_batch(sdf_ctx *ctx, const sdf_anchor_pair *pairs, size_t n, const char *seq_pool,
                                 size_t pool_bytes, int kmer, sdf_anchor *out, size_t out_cap, int64_t *out_off,
                                 size_t *out_used) {
  return sdf_anchors_batch_strand(ctx, pairs, nullptr, n, seq_pool, pool_bytes, kmer, out, out_cap, out_off, out_used);
}

extern "C" int sdf_anchors_batch_view_strand(sdf_ctx *ctx, const sdf_anchor_pair *pairs, const uint8_t *r_rc, size_t n, const char *seq_pool,
                                             size_t pool_bytes, int kmer, const sdf_anchor **out, int64_t *out_off, size_t *out_used) {
  if (!ctx || !out) return SDF_ERR_INVALID;
  *out = nullptr;
  if (hipSetDevice(ctx->device) != hipSuccess || ctx->host_an.reserve_pinned(ctx->cfg.pin_register >= 2, (size_t)48 << 20) != hipSuccess) {
    (void)hipGetLastError();
    ctx->err = "cannot pin the anchors' staging";
    return SDF_ERR_NOMEM;
  }
  int rc = sdf_anchors_batch_strand(ctx, pairs, r_rc, n, seq_pool, pool_bytes, kmer, (sdf_anchor *)ctx->host_an.p, ctx->host_an.cap / sizeof(sdf_anchor),
                             out_off, out_used);
  if (rc == SDF_ERR_CIGAR_OVERFLOW) {  // more anchors than the staging holds: once more with room for all of them
    if (ctx->host_an.reserve_pinned(ctx->cfg.pin_register >= 2, (*out_used + 1024) * sizeof(sdf_anchor)) != hipSuccess) {
      (void)hipGetLastError();
      ctx->err = "cannot pin the anchors' staging";
      return SDF_ERR_NOMEM;
    }
    // (the characters are resident since the first attempt)
    rc = sdf_anchors_batch_strand(ctx, pairs, r_rc, n, nullptr, pool_bytes, kmer, (sdf_anchor *)ctx->host_an.p, ctx->host_an.cap / sizeof(sdf_anchor),
                           out_off, out_used);
  }
  if (rc == SDF_OK) *out = (const sdf_anchor *)ctx->host_an.p;
  return rc;
}

extern "C" int sdf_anchors_batch_view(sdf_ctx *ctx, const sdf_anchor_pair *pairs, size_t n, const char *seq_pool, size_t pool_bytes,
                                      int kmer, const sdf_anchor **out, int64_t *out_off, size_t *out_used) {
  return sdf_anchors_batch_view_strand(ctx, pairs, nullptr, n, seq_pool, pool_bytes, kmer, out, out_off, out_used);
}

// ... of MORE pairs of the resident pool, written behind the first `keep` anchors of the staging (which stay where they are: a
// caller that is still reading them -- the stage driver chains the first half of a super-batch while the device finds the
// anchors of the second -- is not disturbed).  No growth: SDF_ERR_CIGAR_OVERFLOW when the staging has no room for them.
extern "C" int sdf_anchors_batch_more_strand(sdf_ctx *ctx, const sdf_anchor_pair *pairs, const uint8_t *r_rc, size_t n, size_t pool_bytes,
                                             int kmer, size_t keep, const sdf_anchor **out, int64_t *out_off, size_t *out_used) {
  if (!ctx || !out) return SDF_ERR_INVALID;
  *out = nullptr;
  const size_t cap = ctx->host_an.cap / sizeof(sdf_anchor);
  if (!ctx->host_an.p || keep > cap || !pool_bytes) {
    ctx->err = "sdf_anchors_batch_more follows sdf_anchors_batch_view on a resident pool";
    return SDF_ERR_INVALID;
  }
  sdf_anchor *at = (sdf_anchor *)ctx->host_an.p + keep;
  const int rc = sdf_anchors_batch_strand(ctx, pairs, r_rc, n, nullptr, pool_bytes, kmer, at, cap - keep, out_off, out_used);
  if (rc == SDF_OK) *out = at;
  return rc;
}

extern "C" int sdf_anchors_batch_more(sdf_ctx *ctx, const sdf_anchor_pair *pairs, size_t n, size_t pool_bytes, int kmer, size_t keep,
                                      const sdf_anchor **out, int64_t *out_off, size_t *out_used) {
  return sdf_anchors_batch_more_strand(ctx, pairs, nullptr, n, pool_bytes, kmer, keep, out, out_off, out_used);
}

// ---- anchor chaining (reference: src/chain.cc:103-199) ---------------------------------------------------
extern "C" int sdf_chain_batch(sdf_ctx *ctx, const sdf_anchor *anchors, const int64_t *off, size_t n, int max_chain_gap,
                               int match_chain_score, int32_t *path, int32_t *bounds, int32_t *nbound) {
  if (!ctx) return SDF_ERR_INVALID;
  ctx->err.clear();
  if (!off || !bounds || !nbound || n >= (1u << 24)) {
    ctx->err = "invalid arguments";
    return SDF_ERR_INVALID;
  }
  std::fill(ctx->chain_classes, ctx->chain_classes + 7, (int64_t)0);  // (sdf_last_chain_classes: this call's; [7] stays)
  if (n == 0) return SDF_OK;
  // Round 4: a pair whose arrays fit the LDS of a workgroup is swept by ONE WAVEFRONT with everything in LDS
  // (chain_wave_kernel: launch classes by LDS size, the pairs of most anchors first); the others keep the thread-per-pair
  // kernel with its scratch in HBM.  SDF_CHAIN_THREADS=1: every pair on the latter (tests).
  const bool threads_only = ctx->cfg.chain_threads_only != 0;
  // (classes of up to 32 KiB, ~400 anchors, whatever their number; up to the device's LDS per workgroup when they are FEW: a wavefront
  // sweeps an anchor in ~14 us where a thread chasing nodes in HBM takes ~85 -- the launch is its largest pair --, but two
  // such workgroups fit a CU: 8,192 pairs of ~700 anchors take 150 ms that way against 59 ms with every pair in flight on
  // the thread-per-pair kernel; profiles/r04_chain_bench.txt)
  const size_t caps[6] = {2048, 4096, 8192, 16384, 32768, (size_t)ctx->chain_classes[7]};
  std::vector<int32_t> cls[7];  // [6]: thread-per-pair
  std::vector<int64_t> ws_off(n + 1);
  int64_t words = 0;
  for (size_t i = 0; i < n; i++) {
    const int64_t m = off[i + 1] - off[i];
    if (off[0] != 0 || m < 0 || m >= (1 << 26)) {
      ctx->err = "anchor offsets must start at 0, ascend, and hold fewer than 2^26 anchors per pair";
      return SDF_ERR_INVALID;
    }
    ws_off[i] = words;
    int c = 6;
    if (!threads_only && m < (1 << 20)) {
      const size_t need = sdf::chain_wave_lds_bytes((int)m);
      for (int q = 5; q >= 0; --q)
        if (need <= caps[q]) c = q;
    }
    cls[c].push_back((int32_t)i);
    if (c == 6 && m > 0) {
      int bits = 0;
      for (unsigned v = (unsigned)m - 1u; v; v >>= 1) ++bits;
      words += 12 * m + 4 * ((int64_t)2 << bits);
    }
  }
  if (cls[5].size() > 512) {  // many large pairs: every one of them in flight instead
    for (int32_t i : cls[5]) {
      const int64_t m = off[i + 1] - off[i];
      int bits = 0;
      for (unsigned v = (unsigned)m - 1u; v; v >>= 1) ++bits;
      ws_off[i] = words;
      words += 12 * m + 4 * ((int64_t)2 << bits);
    }
    cls[6].insert(cls[6].end(), cls[5].begin(), cls[5].end());
    cls[5].clear();
  }
  ws_off[n] = words;
  for (int c = 0; c < 7; ++c) ctx->chain_classes[c] = (int64_t)cls[c].size();
  std::vector<int32_t> which;
  size_t cls_first[7];
  for (int c = 0; c < 7; ++c) {
    std::stable_sort(cls[c].begin(), cls[c].end(), [&](int32_t a, int32_t b) { return off[a + 1] - off[a] > off[b + 1] - off[b]; });
    cls_first[c] = which.size();
    which.insert(which.end(), cls[c].begin(), cls[c].end());
  }
  const size_t total = (size_t)off[n];
  if (total && (!anchors || !path)) {
    ctx->err = "invalid arguments";
    return SDF_ERR_INVALID;
  }
  SDF_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  SDF_HIP(ctx->ch_an.reserve(total * sizeof(sdf_anchor) + 16));
  SDF_HIP(ctx->ch_off.reserve((n + 1) * 8));
  SDF_HIP(ctx->ch_wsoff.reserve((n + 1) * 8));
  SDF_HIP(ctx->ch_work.reserve((size_t)words * 4 + 16));
  SDF_HIP(ctx->ch_path.reserve(total * 4 + 16));
  SDF_HIP(ctx->ch_bounds.reserve((total + n) * 8));
  SDF_HIP(ctx->ch_nb.reserve(n * 4));
  if (total) SDF_HIP(hipMemcpyAsync(ctx->ch_an.p, anchors, total * sizeof(sdf_anchor), hipMemcpyHostToDevice, st));
  SDF_HIP(hipMemcpyAsync(ctx->ch_off.p, off, (n + 1) * 8, hipMemcpyHostToDevice, st));
  SDF_HIP(hipMemcpyAsync(ctx->ch_wsoff.p, ws_off.data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
  SDF_HIP(ctx->ch_which.reserve(n * 4 + 16));
  SDF_HIP(hipMemcpyAsync(ctx->ch_which.p, which.data(), n * 4, hipMemcpyHostToDevice, st));
  for (int c = 0; c < 6; ++c)
    if (!cls[c].empty())
      hipLaunchKernelGGL(sdf::chain_wave_kernel, dim3((unsigned)cls[c].size()), dim3(64), caps[c], st,
                         (const sdf_anchor *)ctx->ch_an.p, (const int64_t *)ctx->ch_off.p,
                         (const int32_t *)ctx->ch_which.p + cls_first[c], max_chain_gap, match_chain_score,
                         (int32_t *)ctx->ch_path.p, (int32_t *)ctx->ch_bounds.p, (int32_t *)ctx->ch_nb.p);
  if (!cls[6].empty())
    hipLaunchKernelGGL(sdf::chain_kernel, dim3((unsigned)((cls[6].size() + 63) / 64)), dim3(64), 0, st,
                       (const sdf_anchor *)ctx->ch_an.p, (const int64_t *)ctx->ch_off.p, (const int64_t *)ctx->ch_wsoff.p,
                       (int)cls[6].size(), max_chain_gap, match_chain_score, (int32_t *)ctx->ch_work.p, (int32_t *)ctx->ch_path.p,
                       (int32_t *)ctx->ch_bounds.p, (int32_t *)ctx->ch_nb.p, (const int32_t *)ctx->ch_which.p + cls_first[6]);
  SDF_HIP(hipGetLastError());
  if (total) SDF_HIP(hipMemcpyAsync(path, ctx->ch_path.p, total * 4, hipMemcpyDeviceToHost, st));
  SDF_HIP(hipMemcpyAsync(bounds, ctx->ch_bounds.p, (total + n) * 8, hipMemcpyDeviceToHost, st));
  SDF_HIP(hipMemcpyAsync(nbound, ctx->ch_nb.p, n * 4, hipMemcpyDeviceToHost, st));
  SDF_HIP(hipStreamSynchronize(st));
  return SDF_OK;
}

// Test hook: a script of tree operations on chain.hip's device tree (host buffers; one GPU thread).  Returns the number
// of tree nodes (state[i] = node i's p pointer, i < min(nodes, state_cap)) or a negative error code.
extern "C" int sdf_debug_chain_tree_script(sdf_ctx *ctx, const int32_t *pts, int n, const int32_t *ops, int nops, int32_t *out,
                                           int32_t *state, int state_cap) {
  if (!ctx || !pts || n < 1 || nops < 0 || (nops && (!ops || !out))) return SDF_ERR_INVALID;
  ctx->err.clear();
  int bits = 0;
  for (unsigned v = (unsigned)n - 1u; v; v >>= 1) ++bits;
  const int size = (1 << bits) << 1;
  SDF_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const size_t w_pts = (size_t)2 * n, w_ops = (size_t)5 * std::max(nops, 1), w_work = (size_t)4 * n + (size_t)4 * size,
               w_out = (size_t)2 * std::max(nops, 1);
  SDF_HIP(ctx->ch_work.reserve((w_pts + w_ops + w_work + w_out + size) * 4 + 64));
  int32_t *d = (int32_t *)ctx->ch_work.p;
  int32_t *d_pts = d, *d_ops = d_pts + w_pts, *d_work = d_ops + w_ops, *d_out = d_work + w_work, *d_state = d_out + w_out;
  SDF_HIP(hipMemcpyAsync(d_pts, pts, w_pts * 4, hipMemcpyHostToDevice, st));
  if (nops) SDF_HIP(hipMemcpyAsync(d_ops, ops, (size_t)5 * nops * 4, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(sdf::chain_tree_script_kernel, dim3(1), dim3(64), 0, st, d_pts, n, d_ops, nops, d_work, size, d_out, d_state);
  SDF_HIP(hipGetLastError());
  if (nops) SDF_HIP(hipMemcpyAsync(out, d_out, (size_t)2 * nops * 4, hipMemcpyDeviceToHost, st));
  if (state && state_cap > 0)
    SDF_HIP(hipMemcpyAsync(state, d_state, (size_t)std::min(size, state_cap) * 4, hipMemcpyDeviceToHost, st));
  SDF_HIP(hipStreamSynchronize(st));
  return size;
}
