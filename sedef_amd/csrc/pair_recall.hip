// Pair recall (include/sedef_hip.h: sdf_pair_recall): per gold record the found records that hit it and the bases of its two
// ends they cover -- `sedef stats recall`, the join the reference leaves to `bedtools pairtopair -type both` and a numpy array
// per base (scratch/check-overlap.py).  The rule itself is sdf_kernels.h's (recall_meets, recall_entry, recall_clip), shared
// with the host form.
//
// The index is a SORT, not bins: chromosome ids are the caller's and need not be dense, and the one figure a sorted list needs
// to be searched by overlap -- the longest end -- is a single atomic maximum.
//   recall_entries_kernel   a lane a found record: an entry per end, key recall_key(chromosome, start), value 2 * record + end;
//                           an end without a base, and both ends of a record the checks refuse (counted in status[0]), get
//                           kRecallNoKey, which sorts behind every key a gold end asks for; one atomic maximum a wavefront
//                           into *max_len.
//   the library's radix sort of the entries by key;
//   recall_kernel           a workgroup of ONE wavefront a gold record.  Two wave-wide bound searches give the entries that can
//                           meet end 1 (sdf_kernels.h: the candidates); the lanes walk them 64 at a time, each loads its entry's
//                           record and applies recall_entry, and the hits' two clipped intervals are compacted by ballot into
//                           two LDS lists of kRecallCap.  A list's union length: the bitonic sort of chain.hip on
//                           start << 32 | end, then a running maximum of the ends -- an interval adds what lies behind the
//                           largest end in front of it.  n_hits needs no list and is exact however many hits there are; more
//                           list entries than kRecallCap set SDF_RECALL_WIDE and leave the coverage 0 (the caller's to finish).
// LDS: 2 * kRecallCap * 8 = 16 KiB a workgroup of one wavefront, so ten wavefronts a CU (the compiler's figure: 3 a SIMD) where the
// registers would allow more.  The walk waits on gathers of 32-byte records, which is what more wavefronts would hide; a larger
// cap would buy fewer WIDE records with fewer wavefronts.
#include <hip/hip_runtime.h>

#include "search_dev.h"

namespace sdf {

__global__ __launch_bounds__(256) void recall_entries_kernel(const sdf_pair_rec *__restrict__ found, int nf, unsigned long long *__restrict__ keys,
                                                             uint32_t *__restrict__ vals, int32_t *__restrict__ max_len,
                                                             unsigned long long *__restrict__ status) {
  const int id = blockIdx.x * 256 + threadIdx.x;
  int longest = 0;
  bool bad = false;
  if (id < nf) {
    const sdf_pair_rec F = found[id];
    bad = recall_rec_bad(F);
#pragma unroll
    for (int e = 0; e < 2; e++) {
      const RecallEnd E = recall_end(F, e);
      const bool live = !bad && E.end > E.start;
      keys[2 * (size_t)id + e] = live ? recall_key(E.chr, E.start) : kRecallNoKey;
      vals[2 * (size_t)id + e] = 2u * (uint32_t)id + (uint32_t)e;
      if (live && E.end - E.start > longest) longest = E.end - E.start;
    }
  }
#pragma unroll
  for (int d = 32; d; d >>= 1) {
    const int o = __shfl_xor(longest, d, 64);
    longest = o > longest ? o : longest;
  }
  const unsigned long long n_bad = __popcll(__ballot(bad));
  if ((threadIdx.x & 63) == 0) {
    if (longest) (void)__hip_atomic_fetch_max(max_len, longest, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (n_bad) (void)__hip_atomic_fetch_add(status, n_bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ascending sort of a[0 .. n) in LDS by the workgroup's single wavefront: chain_sort_u64's network (chain.hip)
__device__ __forceinline__ void recall_sort_u64(unsigned long long *a, const int n, const int lane) {
  int np2 = 1;
  while (np2 < n) np2 <<= 1;
  for (int k = 2; k <= np2; k <<= 1) {
    for (int idx = lane; idx < np2 / 2; idx += 64) {
      const int blk = idx / (k / 2), off = idx % (k / 2);
      const int i = blk * k + off, j = blk * k + k - 1 - off;
      if (j < n) {
        const unsigned long long x = a[i], y = a[j];
        if (x > y) a[i] = y, a[j] = x;
      }
    }
    __syncthreads();
    for (int jj = k / 4; jj >= 1; jj >>= 1) {
      for (int idx = lane; idx < np2 / 2; idx += 64) {
        const int i = (idx / jj) * 2 * jj + idx % jj, j = i + jj;
        if (j < n) {
          const unsigned long long x = a[i], y = a[j];
          if (x > y) a[i] = y, a[j] = x;
        }
      }
      __syncthreads();
    }
  }
}

// the bases of [0, ...) inside the union of the intervals a[0 .. n) (start << 32 | end, 1 <= n <= kRecallCap); sorts a[] in place
__device__ __forceinline__ int recall_union(unsigned long long *a, const int n, const int lane) {
  recall_sort_u64(a, n, lane);
  int total = 0, reach = 0;  // reach: the largest end of the intervals in front of this round's
  for (int s0 = 0; s0 < n; s0 += 64) {
    const int s = s0 + lane;
    const unsigned long long iv = s < n ? a[s] : 0ull;
    const int start = (int)(iv >> 32), end = (int)(iv & 0xFFFFFFFFull);
    int upto = end;  // the largest end of this round's intervals up to this lane's
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(upto, d, 64);
      if (lane >= d && o > upto) upto = o;
    }
    int before = __shfl_up(upto, 1, 64);
    if (lane == 0 || before < reach) before = reach;
    const int from = start > before ? start : before;
    total += stats_wave_sum(end > from ? end - from : 0);
    const int last = __builtin_amdgcn_readlane(upto, 63);
    reach = last > reach ? last : reach;
  }
  return total;
}

__global__ __launch_bounds__(64) void recall_kernel(const sdf_pair_rec *__restrict__ gold, const sdf_pair_rec *__restrict__ found,
                                                    const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ vals, int n_ent,
                                                    const int32_t *__restrict__ max_len_p, uint32_t flags, sdf_pair_recall_rec *__restrict__ out,
                                                    unsigned long long *__restrict__ status) {
  __shared__ unsigned long long list1[kRecallCap], list2[kRecallCap];
  const int lane = threadIdx.x;
  const size_t g = blockIdx.x;
  const sdf_pair_rec G = gold[g];
  if (recall_rec_bad(G)) {  // (the whole workgroup)
    if (lane == 0) {
      out[g] = sdf_pair_recall_rec{0u, 0, 0, SDF_RECALL_BAD};
      (void)__hip_atomic_fetch_add(status + 1, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return;
  }
  const bool ignore_strand = (flags & SDF_RECALL_IGNORE_STRAND) != 0;
  const int max_len = *max_len_p;
  long long n_list = 0;
  uint32_t n_hits = 0;
  if (G.end1 > G.start1 && G.end2 > G.start2 && max_len > 0 && n_ent > 0) {
    const unsigned long long key_lo = recall_key(G.chr1, (long long)G.start1 - max_len + 1), key_hi = recall_key(G.chr1, G.end1);
    const int k_lo = search_wave_bound(n_ent, [&](int x) { return keys[x] < key_lo; }, lane);
    const int k_hi = search_wave_bound(n_ent, [&](int x) { return keys[x] < key_hi; }, lane);
    for (long long base = k_lo; base < k_hi; base += 64) {
      const long long k = base + lane;
      bool hit = false, counts = false;
      unsigned long long iv1 = 0, iv2 = 0;
      if (k < k_hi) {
        const uint32_t v = vals[k];
        recall_entry(G, found[v >> 1], (int)(v & 1u), ignore_strand, &hit, &counts, &iv1, &iv2);
      }
      const unsigned long long m = __ballot(hit);
      const long long at = n_list + __popcll(m & ((1ull << lane) - 1ull));
      if (hit && at < kRecallCap) list1[at] = iv1, list2[at] = iv2;
      n_list += __popcll(m);
      n_hits += (uint32_t)__popcll(__ballot(counts));
    }
  }
  const bool wide = n_list > kRecallCap;
  int cov1 = 0, cov2 = 0;
  if (!wide && n_list > 0) {  // (wave-uniform: every lane reaches the barriers)
    __syncthreads();
    cov1 = recall_union(list1, (int)n_list, lane);
    cov2 = recall_union(list2, (int)n_list, lane);
  }
  if (lane == 0) out[g] = sdf_pair_recall_rec{n_hits, cov1, cov2, wide ? SDF_RECALL_WIDE : 0u};
}

}  // namespace sdf
