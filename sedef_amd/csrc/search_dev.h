// Device helpers the search kernels share (search_seeds.hip, search_roll.hip, search_extend.hip): a workgroup is ONE wavefront, its keys lie in LDS.
// The `_wg` forms at the end serve search_seeds_wide.hip, whose workgroup is several wavefronts: they take the thread index and
// the thread count, and every lane of the workgroup calls them together.
#pragma once
#include <hip/hip_runtime.h>

#include "sdf_kernels.h"
#include "stats_dev.h"

namespace sdf {

// a loc as a sort key whose unsigned order is the locs' signed order, and back; kSearchGone: a filtered loc (sorts last)
constexpr uint32_t kSearchGone = 0xFFFFFFFFu;
__device__ __forceinline__ uint32_t search_loc_key(int loc) { return (uint32_t)loc ^ 0x80000000u; }
__device__ __forceinline__ long long search_key_loc(uint32_t k) { return (long long)(int)(k ^ 0x80000000u); }

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

// A key of the roll and the extension in 32 bits: status << 30 | hash (hash < 2^30: the header's contract).
__device__ __forceinline__ uint32_t roll_key(const sdf_minimizer &M) { return ((uint32_t)M.status & 3u) << 30 | (M.hash & 0x3FFFFFFFu); }

// the slot of a key that is among keys[0 .. nd)
__device__ __forceinline__ int roll_slot(const uint32_t *keys, const int nd, const uint32_t key) {
  int lo = 0, hi = nd - 1;
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (keys[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// The sort and the slots of the keys in keys[0 .. n): keys[0 .. nd) are the distinct keys in ascending order and bits[] is 0 on
// them afterwards; returns nd.  (The caller looks its records' slots up with roll_slot and syncs before it reuses keys[].)
__device__ __forceinline__ int search_slots_setup(uint32_t *keys, uint8_t *bits, const int n, const int lane) {
  __syncthreads();
  search_sort_u32(keys, n, lane);
  const int nd = search_compact_u32(keys, n, lane);
  for (int x = lane; x < nd; x += 64) bits[x] = 0;
  __syncthreads();
  return nd;
}

// The SlidingMap of include/sedef_hip.h over slots: bits[slot], the boundary slot B (-1: none) and the counter I.  Wave-uniform:
// every lane carries B and I and makes every write to bits[] itself, so a lane reads back only what it wrote and nothing here
// needs a barrier.  The boundary's predecessor and successor are the one place the lanes share work: 64 neighbouring slots a
// round, a ballot over bits != 0.
struct SearchMap {
  uint8_t *bits;
  int nd, B, I;
  __device__ __forceinline__ int bit(const int sl) const { return __builtin_amdgcn_readfirstlane((int)bits[sl]); }
  __device__ __forceinline__ bool full(const int sl) const { return sl >= 0 && bit(sl) == 3; }
  // the largest stored slot below b (-1: none), the smallest above b (nd: none)
  __device__ __forceinline__ int below(const int b, const int lane) const {
    for (int base = b - 1; base >= 0; base -= 64) {
      const int x = base - lane;
      const unsigned long long m = __ballot(x >= 0 && bits[x] != 0);
      if (m) return base - __builtin_ctzll(m);
    }
    return -1;
  }
  __device__ __forceinline__ int above(const int b, const int lane) const {
    for (int base = b + 1; base < nd; base += 64) {
      const int x = base + lane;
      const unsigned long long m = __ballot(x < nd && bits[x] != 0);
      if (m) return base + __builtin_ctzll(m);
    }
    return nd;
  }
  // add(k, BIT) and remove(k, BIT) of the header; counted: query_size != 0
  __device__ __forceinline__ bool add(const int sl, const int BIT, const bool counted, const int lane) {
    const int b = bit(sl);
    if (b & BIT) return false;
    bits[sl] = (uint8_t)(b | BIT);
    if (counted && sl < B) {
      I += (b | BIT) == 3 ? 1 : 0;
      if (b == 0) {
        I -= full(B) ? 1 : 0;
        B = below(B, lane);  // sl at the latest
      }
    }
    return true;
  }
  __device__ __forceinline__ bool remove(const int sl, const int BIT, const bool counted, const int lane) {
    const int b = bit(sl);
    if (!(b & BIT)) return false;
    if (counted && sl <= B) {
      I -= b == 3 ? 1 : 0;
      if (b == BIT) {
        const int up = above(B, lane);
        if (up < nd) {
          B = up;
          I += full(B) ? 1 : 0;
        }
      }
    }
    bits[sl] = (uint8_t)(b & ~BIT);
    return true;
  }
};

// The roll's walk (include/sedef_hip.h, steps 1 to 5) over the span's records x = 0 .. nspan): slot[x] (NO_SLOT: status 2) and
// locs[x] -- pointers into LDS (search_roll.hip, search_extend.hip), or anything else with a wave-uniform operator[]
// (search_extend_long.hip: windows on HBM).  It jumps from event to event (a step without one cannot change J).
// eval(s, e, ws, we) is called at every evaluation of J -- step 4 and every round with an event -- and ends the walk by returning
// true.  ws, we count from the span's first record.
template <int NO_SLOT = 0xFFFF, class Slots, class Locs, class F>
__device__ __forceinline__ void search_roll_walk(SearchMap &S, Slots slot, Locs locs, const int nspan, const long long start,
                                                 const long long end, const int init_len, const long long len_r, const int lane, F eval) {
  constexpr int no_slot = NO_SLOT;
  auto add = [&](int x) {
    const int sl = __builtin_amdgcn_readfirstlane((int)slot[x]);
    if (sl != no_slot) S.add(sl, 2, true, lane);
  };
  auto remove = [&](int x) {
    const int sl = __builtin_amdgcn_readfirstlane((int)slot[x]);
    if (sl != no_slot) S.remove(sl, 2, true, lane);
  };
  long long s = start, e = start + init_len < len_r ? start + init_len : len_r;
  int ws = 0, we = 0;
  while (we < nspan && (long long)locs[we] < e) add(we++);
  if (eval(s, e, ws, we)) return;
  while (s < end && e < len_r) {  // (e was not clamped: e == s + init_len)
    // the next step with an event: a remove at the first s' >= s with loc <= s', an add at loc == s' + init_len
    long long next = -1;
    if (ws < nspan) next = (long long)locs[ws] > s ? (long long)locs[ws] : s;
    if (we < nspan && (long long)locs[we] >= e) {
      const long long at = (long long)locs[we] - init_len;
      next = next < 0 || at < next ? at : next;
    }
    if (next < 0 || next >= end || next + init_len >= len_r) break;
    s = next, e = next + init_len;
    if (ws < nspan && (long long)locs[ws] <= s) remove(ws++);
    if (we < nspan && (long long)locs[we] == e) add(we++);
    if (eval(s, e, ws, we)) return;
    s++, e++;
  }
}

// ---- a workgroup of nt lanes (a multiple of 64), tid its thread index ----

// The exclusive prefix sum of v over the workgroup, *all its sum: stats_wave_scan inside a wavefront, the wavefronts' totals
// through ws[0 .. nt / 64) in LDS.  Two barriers: what the lanes read before the call is read before anything written after it.
__device__ __forceinline__ int search_wg_scan(const int v, int *all, int *ws, const int tid, const int nt) {
  const int in = stats_wave_scan(v), wave = tid >> 6;
  __syncthreads();  // (ws[] of the call before has been read)
  if ((tid & 63) == 63) ws[wave] = in;
  __syncthreads();
  int before = 0, sum = 0;
  for (int k = 0; k < nt >> 6; k++) {
    const int s = ws[k];
    before += k < wave ? s : 0;
    sum += s;
  }
  *all = sum;
  return before + in - v;
}

// the exact sum of v over the workgroup, through ws[0 .. nt / 64)
__device__ __forceinline__ long long search_wg_sum64(const long long v, long long *ws, const int tid, const int nt) {
  long long s = v;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
  __syncthreads();
  if ((tid & 63) == 0) ws[tid >> 6] = s;
  __syncthreads();
  long long sum = 0;
  for (int k = 0; k < nt >> 6; k++) sum += ws[k];
  return sum;
}

// search_sort_u32 by the whole workgroup: the same network, nt compare-exchanges a step
__device__ __forceinline__ void search_sort_u32_wg(uint32_t *a, const int n, const int tid, const int nt) {
  int np2 = 1;
  while (np2 < n) np2 <<= 1;
  for (int k = 2; k <= np2; k <<= 1) {
    for (int idx = tid; idx < np2 / 2; idx += nt) {
      const int blk = idx / (k / 2), off = idx % (k / 2);
      const int i = blk * k + off, j = blk * k + k - 1 - off;
      if (j < n) {
        const uint32_t x = a[i], y = a[j];
        if (x > y) a[i] = y, a[j] = x;
      }
    }
    __syncthreads();
    for (int jj = k / 4; jj >= 1; jj >>= 1) {
      for (int idx = tid; idx < np2 / 2; idx += nt) {
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

// search_compact_u32 by the whole workgroup, nt keys a round: a round reads its keys and the one in front of them before it
// writes (search_wg_scan's barriers), and never writes behind what it read -- the key in front of a round, c[s0 - 1], is either
// untouched by the rounds before or was rewritten with itself (every key before it was distinct).  Returns the distinct keys.
__device__ __forceinline__ int search_compact_u32_wg(uint32_t *c, const int nv, int *ws, const int tid, const int nt) {
  int nc = 0;
  for (int s0 = 0; s0 < nv; s0 += nt) {
    const int s = s0 + tid;
    const bool in = s < nv;
    const uint32_t mine = in ? c[s] : 0u, left = in && s > 0 ? c[s - 1] : 0u;
    const bool fresh = in && (s == 0 || mine != left);
    int all;
    const int at = search_wg_scan(fresh ? 1 : 0, &all, ws, tid, nt);
    if (fresh) c[nc + at] = mine;
    nc += all;
    __syncthreads();
  }
  return nc;
}

}  // namespace sdf
