// Line order (include/sedef_hip.h: sdf_line_order): text lines by eight keys and, inside a run of equal keys, by their bytes, with
// the duplicates flagged -- the two `sort -k1,1V -k9,9r ... | uniq` passes between `align generate` and final.bed
// (sedef.sh:218-229; `sedef report`, host/report_cmd.cc).  The keys are the host's (ranks and values, ascending); what is left
// for the device is a stable sort of records and the one step that has to read the long lines: ordering and comparing the lines
// that share all eight keys, which is where the same alignment out of several overlapping buckets meets itself.
//   line_keys_kernel    a lane a place: the 64-bit composite of one pair of keys of the line that stands there -- the sort key
//                       of one of the four stable radix passes, least significant pair first.  The first pass (no places yet)
//                       writes the identity and counts the lines the checks refuse (sdf_kernels.h: line_rec_bad).
//   line_heads_kernel   a lane a place, behind the last pass: whether a run starts there, flags cleared, and the starts of the
//                       runs of two lines and more appended to a list, one atomic a wavefront (the list's order is of no
//                       consequence: runs do not share places).
//   line_tie_kernel     a workgroup of ONE wavefront a listed run.  The run's length is a ballot over the next 64 head bytes.
//                       Up to kLineRun lines: offsets, lengths and indices go to LDS, and every pair of lines is compared by the
//                       whole wavefront, 16 bytes a lane a step (1 KiB a step, one global_load_dwordx4 a line: `off` is a
//                       multiple of 16); each lane finds the first byte of its sixteen that differs inside the common length,
//                       a ballot finds the first such lane, and that lane's two bytes decide, unsigned.  Without a difference
//                       the shorter line is the smaller.  A line's rank inside the run is the number of lines below it, equal
//                       lines counting for the later index, so identical lines keep their order; a line equal to an earlier
//                       one is a duplicate of its predecessor in the new order.  Longer runs keep index order and get
//                       SDF_LINE_WIDE on every place.
// LDS: 1.5 KiB a workgroup.  A run of m lines costs m (m - 1) / 2 comparisons; the runs `align generate` leaves are the copies
// of one alignment, two to a handful.
#include <hip/hip_runtime.h>

#include "sdf_kernels.h"

namespace sdf {

__global__ __launch_bounds__(256) void line_keys_kernel(const sdf_line_rec *__restrict__ lines, const uint32_t *__restrict__ place_in,
                                                        uint32_t *__restrict__ place_out, unsigned long long *__restrict__ keys, int n, int pair,
                                                        unsigned long long pool_bytes, uint32_t *__restrict__ counts) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  bool bad = false;
  if (p < n) {
    const uint32_t i = place_in ? place_in[p] : (uint32_t)p;
    const sdf_line_rec &L = lines[i];
    keys[p] = (unsigned long long)L.key[2 * pair] << 32 | L.key[2 * pair + 1];
    if (!place_in) {
      place_out[p] = i;
      bad = line_rec_bad(L, pool_bytes);
    }
  }
  if (!place_in) {  // (the whole grid)
    const uint32_t n_bad = (uint32_t)__popcll(__ballot(bad));
    if ((threadIdx.x & 63) == 0 && n_bad) (void)__hip_atomic_fetch_add(counts + 2, n_bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ __launch_bounds__(256) void line_heads_kernel(const sdf_line_rec *__restrict__ lines, const uint32_t *__restrict__ order, int n,
                                                         uint8_t *__restrict__ head, uint32_t *__restrict__ flags, uint32_t *__restrict__ run_start,
                                                         uint32_t *__restrict__ n_runs, uint32_t *__restrict__ counts) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  bool starts = false;
  if (p < n) {
    const sdf_line_rec &me = lines[order[p]];
    const bool h = p == 0 || !line_keys_equal(lines[order[p - 1]], me);
    const bool next_h = p + 1 >= n || !line_keys_equal(me, lines[order[p + 1]]);
    head[p] = h ? 1 : 0;
    flags[p] = 0u;
    starts = h && !next_h;
    if (p == 0) (void)__hip_atomic_fetch_add(counts, (uint32_t)n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (the tie kernel takes the duplicates off)
  }
  const unsigned long long m = __ballot(starts);
  if (m) {  // (wave-uniform)
    const int first = __ffsll((long long)m) - 1;
    uint32_t base = 0;
    if (lane == first) base = __hip_atomic_fetch_add(n_runs, (uint32_t)__popcll(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    base = __shfl(base, first, 64);
    if (starts) run_start[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = (uint32_t)p;
  }
}

// sixteen bytes of the pool from `at` (a multiple of 16 above a 16-byte aligned base); what lies behind pool_bytes reads as 0
__device__ __forceinline__ uint4 line_load16(const uint8_t *__restrict__ pool, const unsigned long long at, const unsigned long long pool_bytes) {
  if (at + 16 <= pool_bytes) return *reinterpret_cast<const uint4 *>(pool + at);
  uint32_t w[4] = {0u, 0u, 0u, 0u};
  for (int b = 0; b < 16; b++)
    if (at + (unsigned long long)b < pool_bytes) w[b >> 2] |= (uint32_t)pool[at + (unsigned long long)b] << (8 * (b & 3));
  return make_uint4(w[0], w[1], w[2], w[3]);
}

// memcmp order of two lines by the whole wavefront: below 0, 0, above 0 (wave-uniform)
__device__ __forceinline__ int line_compare(const uint8_t *__restrict__ pool, const unsigned long long pool_bytes, const unsigned long long off_a,
                                            const uint32_t len_a, const unsigned long long off_b, const uint32_t len_b, const int lane) {
  const unsigned long long common = len_a < len_b ? len_a : len_b;
  for (unsigned long long base = 0; base < common; base += 1024) {
    const unsigned long long c = base + 16ull * (unsigned long long)lane;
    uint32_t first = 16u, byte_a = 0u, byte_b = 0u;  // this lane's first differing byte inside the common length, and its two values
    if (c < common) {
      const uint4 A = line_load16(pool, off_a + c, pool_bytes), B = line_load16(pool, off_b + c, pool_bytes);
      const uint32_t valid = common - c < 16ull ? (uint32_t)(common - c) : 16u;
      const uint32_t a[4] = {A.x, A.y, A.z, A.w}, b[4] = {B.x, B.y, B.z, B.w};
#pragma unroll
      for (int w = 3; w >= 0; w--) {  // (the lowest word with a difference in a valid byte wins: little-endian, byte 0 first)
        const uint32_t x = a[w] ^ b[w];
        if (x) {
          const uint32_t in_word = (uint32_t)(__ffs((int)x) - 1) >> 3, byte = 4u * (uint32_t)w + in_word;
          if (byte < valid) first = byte, byte_a = (a[w] >> (8u * in_word)) & 255u, byte_b = (b[w] >> (8u * in_word)) & 255u;
        }
      }
    }
    const unsigned long long m = __ballot(first < 16u);
    if (m) {
      const int src = __ffsll((long long)m) - 1;
      const uint32_t va = __shfl(byte_a, src, 64), vb = __shfl(byte_b, src, 64);
      return va < vb ? -1 : 1;
    }
  }
  return len_a < len_b ? -1 : len_a > len_b ? 1 : 0;
}

__global__ __launch_bounds__(64) void line_tie_kernel(const uint8_t *__restrict__ pool, unsigned long long pool_bytes,
                                                      const sdf_line_rec *__restrict__ lines, int n, const uint8_t *__restrict__ head,
                                                      const uint32_t *__restrict__ run_start, const uint32_t *__restrict__ n_runs_p,
                                                      uint32_t *__restrict__ order, uint32_t *__restrict__ flags, uint32_t *__restrict__ counts) {
  __shared__ unsigned long long s_off[kLineRun];
  __shared__ uint32_t s_len[kLineRun], s_idx[kLineRun], s_rank[kLineRun], s_dup[kLineRun];
  const int lane = threadIdx.x;
  const uint32_t n_runs = *n_runs_p;
  for (uint32_t r = blockIdx.x; r < n_runs; r += gridDim.x) {  // (wave-uniform throughout)
    const unsigned long long start = run_start[r];
    // the run's lines stand at start .. start + k, lane k the first whose place start + 1 + k is a head or behind the last place
    const unsigned long long q = start + 1ull + (unsigned long long)lane;
    const unsigned long long stops = __ballot(q >= (unsigned long long)n || head[q] != 0);
    if (stops == 0) {  // more than kLineRun lines: left in index order, every place flagged
      if (lane == 0) (void)__hip_atomic_fetch_add(counts + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      for (unsigned long long base = start;; base += 64) {
        const unsigned long long at = base + (unsigned long long)lane;
        const unsigned long long ends = __ballot(at >= (unsigned long long)n || (at != start && head[at] != 0));
        const unsigned long long below = ends ? (ends & (0ull - ends)) - 1ull : ~0ull;  // the lanes in front of the first end
        if ((below >> lane) & 1ull) flags[at] = SDF_LINE_WIDE;
        if (ends) break;
      }
      continue;
    }
    const int m = __ffsll((long long)stops);  // 2 .. kLineRun lines
    __syncthreads();                          // (the round before has read its LDS)
    if (lane < m) {
      const uint32_t idx = order[start + (unsigned long long)lane];
      const sdf_line_rec L = lines[idx];
      const bool bad = line_rec_bad(L, pool_bytes);  // (counted by line_keys_kernel: a line of no bytes here)
      s_off[lane] = bad ? 0ull : L.off;
      s_len[lane] = bad ? 0u : L.len;
      s_idx[lane] = idx;
      s_rank[lane] = 0u;
      s_dup[lane] = 0u;
    }
    __syncthreads();
    for (int i = 0; i + 1 < m; i++)
      for (int j = i + 1; j < m; j++) {
        const int c = line_compare(pool, pool_bytes, s_off[i], s_len[i], s_off[j], s_len[j], lane);
        if (lane == 0) {
          if (c <= 0) s_rank[j] += 1u;  // (equal lines: the earlier index stays in front)
          else s_rank[i] += 1u;
          if (c == 0) s_dup[j] = 1u;
        }
      }
    __syncthreads();
    bool dup = false;
    if (lane < m) {
      const unsigned long long place = start + s_rank[lane];
      dup = s_dup[lane] != 0u;
      order[place] = s_idx[lane];
      flags[place] = dup ? SDF_LINE_DUP : 0u;
    }
    const uint32_t n_dup = (uint32_t)__popcll(__ballot(dup));
    if (lane == 0 && n_dup) (void)__hip_atomic_fetch_sub(counts, n_dup, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

}  // namespace sdf
