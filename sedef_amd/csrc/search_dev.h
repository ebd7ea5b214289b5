// Device helpers the search kernels share (search_seeds.hip, search_roll.hip): a workgroup is ONE wavefront, its keys lie in LDS.
#pragma once
#include <hip/hip_runtime.h>

#include "sdf_kernels.h"

namespace sdf {

// ascending sort of a[0 .. n) in LDS by the workgroup's single wavefront: chain_sort_u64's network (chain.hip) on 32-bit keys
__device__ __forceinline__ void search_sort_u32(uint32_t *a, const int n, const int lane) {
  int np2 = 1;
  while (np2 < n) np2 <<= 1;
  for (int k = 2; k <= np2; k <<= 1) {
    for (int idx = lane; idx < np2 / 2; idx += 64) {
      const int blk = idx / (k / 2), off = idx % (k / 2);
      const int i = blk * k + off, j = blk * k + k - 1 - off;
      if (j < n) {
        const uint32_t x = a[i], y = a[j];
        if (x > y) a[i] = y, a[j] = x;
      }
    }
    __syncthreads();
    for (int jj = k / 4; jj >= 1; jj >>= 1) {
      for (int idx = lane; idx < np2 / 2; idx += 64) {
        const int i = (idx / jj) * 2 * jj + idx % jj, j = i + jj;
        if (j < n) {
          const uint32_t x = a[i], y = a[j];
          if (x > y) a[i] = y, a[j] = x;
        }
      }
      __syncthreads();
    }
  }
}

// the set of the sorted c[0 .. nv): its distinct keys to the front, in place, 64 at a time (a round reads before it writes, and
// never writes behind what it read); returns their number
__device__ __forceinline__ int search_compact_u32(uint32_t *c, const int nv, const int lane) {
  int nc = 0;
  uint32_t before = 0;  // the key in front of this round's first (not read in the first round)
  for (int s0 = 0; s0 < nv; s0 += 64) {
    const int s = s0 + lane;
    const uint32_t mine = s < nv ? c[s] : 0u;
    const uint32_t left = (uint32_t)__builtin_amdgcn_ds_bpermute((lane - 1) << 2, (int)mine);
    const bool fresh = s < nv && (s == 0 || mine != (lane ? left : before));
    const unsigned long long m = __ballot(fresh);
    before = (uint32_t)__builtin_amdgcn_readlane((int)mine, 63);
    __syncthreads();
    if (fresh) c[nc + __popcll(m & ((1ull << lane) - 1ull))] = mine;
    nc += __popcll(m);
    __syncthreads();
  }
  return nc;
}

// The first x of [0, n) where pred(x) fails, n when it never does; pred holds on a prefix of [0, n).  The wavefront probes 64
// places a round -- four rounds for sixteen million -- where a binary search would wait for one load after the other.  Every
// lane returns the same answer; a pred that holds on no prefix still ends, somewhere inside [0, n].
template <class P>
__device__ __forceinline__ int search_wave_bound(const int n, P pred, const int lane) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int step = (int)(((long long)hi - lo + 63) / 64);
    const long long p = (long long)lo + (long long)lane * step;
    const bool ok = p < hi && pred((int)p);
    const int c = __popcll(__ballot(ok));  // the probes that hold: the first c
    if (c == 0) {
      hi = lo;
    } else {
      const long long next = (long long)lo + (long long)c * step;
      lo = (int)((long long)lo + (long long)(c - 1) * step + 1);
      hi = next < hi ? (int)next : hi;
    }
  }
  return lo;
}

}  // namespace sdf
