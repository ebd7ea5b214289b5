// The winnowed minimizers of ranges of the resident pool, and the index over them: what `sedef search` rests on
// (reference: get_minimizers and Index::Index, src/hash.cc:53-141).
//
// For a sequence s (a range as it lies in the pool, or its reverse complement by rev_dna; characters taken & 127) and k-mer
// starts j = 0 .. nk - 1, nk = len - k + 1:
//   hash(j)    the 2-bit codes of s[j .. j + k), first character most significant (A 0, C 1, G 2, T 3, anything else 0);
//   status(j)  2 if one of the k characters is N / n, else 0 if one is an uppercase letter, else 1 (0 without
//              separate_lowercase);
//   key(j)     (status, hash) as a pair -- here status << 30 | hash in ONE 32-bit word: k <= 15 leaves the hash 30 bits, and
//              unsigned order of the word is the order of the pair;
//   root       j is a root when no y in [max(0, j - w), j) has key(y) < key(j);
//   minimizers the largest root <= w, then every root > w, in loc order; none when nk <= w.
// That is the reference's deque loop in closed form (its second loop tests window.back().loc and pops the front:
// tests/minim_model.py holds the loop as written and checks the two against each other).  Nothing is sequential in it.
//
// One wavefront takes MINIM_BLOCK k-mer starts [b0, e0) of one range.  It needs the keys of [b0 - w, e0) -- the look-back
// of its first start -- hence the characters [b0 - w, e0 + k - 1): a left halo of w, k - 1 to the right.  They are read once, in
// 16-byte units of the pool (a unit that crosses an end of the range is read byte by byte: no byte outside the range is
// touched); a reversed range is read from its far end, each unit byte-swapped and complemented four characters a word
// (stats_revcomp4).  A lane holds one unit: its sixteen codes in a word, an N bit and an uppercase bit per character.  k <= 15
// characters from any of its sixteen starts end in the NEXT lane's unit at the latest, so hash and status of all sixteen come
// from the lane's words and the next lane's (one lane shift of each), by shifts and masks -- no loop over k, and no scan:
// the "last N before here" of the reference's loop is never needed further back than one unit.  Rounds of 64 units overlap by
// one, the last lane of a round only lends its words.  The keys go to LDS (4 bytes a start, MINIM_BLOCK + MINIM_MAX_W of
// them); the root flags are a look-back of w LDS reads per start, 64 consecutive starts a round (consecutive lanes,
// consecutive words: no bank conflict), left as soon as no lane of the round can still be a root.
//
// Launches, in the order stats_cuts.hip established: minim_blocks_kernel (blocks per range; stats_cuts_scan_kernel turns them
// into every range's first block), minim_count_kernel (records per block; the same scan kernel again), minim_first_kernel
// (first[] of the ranges), minim_emit_kernel (the records, in loc order: a block's records start at the scan's offset, the
// rank inside is a ballot count; the block at start 0 writes the "largest root <= w" record first).  A range of any length
// is just more blocks.
//
// The index: records -> keys range << 32 | status << 30 | hash, sorted by the library's radix sort (stable, and the records
// come in loc order: loc needs no bits), heads of equal keys flagged and counted, group sizes sorted per range (the same
// sort), and one lane per range reads its threshold off the sorted sizes (minim_threshold_kernel).
#include <hip/hip_runtime.h>

#include "sdf_kernels.h"
#include "stats_dev.h"

namespace sdf {

// k-mer starts of range R (0 for a range that does not lie in the pool: the host form has refused it, the device form skips it)
__device__ __forceinline__ int minim_starts(const sdf_minim_range &R, long long pool_bytes, int k) {
  if (R.off < 0 || R.len < 0 || R.off > pool_bytes || R.len > pool_bytes - R.off || (R.flags & ~SDF_MINIM_RC)) return 0;
  return R.len >= k ? R.len - k + 1 : 0;
}

// ---- blocks of every range: at least one, so that the ranges' first blocks are strictly ascending ----
__global__ __launch_bounds__(256) void minim_blocks_kernel(const sdf_minim_range *__restrict__ ranges, int n, long long pool_bytes, int k,
                                                           uint32_t *__restrict__ blocks) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int nk = minim_starts(ranges[i], pool_bytes, k);
  blocks[i] = nk ? (uint32_t)((nk - 1) / MINIM_BLOCK + 1) : 1u;
}

struct MinimBlock {  // what a wavefront works on (wave-uniform)
  int range, nk, b0, cnt;  // its range, the range's starts, the block's first start and how many it has
};

// the block of workgroup `blk`: the last range whose first block is not behind it
__device__ __forceinline__ MinimBlock minim_find(const sdf_minim_range *__restrict__ ranges, int n, const uint64_t *__restrict__ blk0,
                                                 long long pool_bytes, int k, uint64_t blk) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = lo + (hi - lo) / 2;
    if (blk0[mid] <= blk) lo = mid;
    else hi = mid;
  }
  MinimBlock B;
  B.range = lo;
  B.nk = minim_starts(ranges[lo], pool_bytes, k);
  B.b0 = (int)(blk - blk0[lo]) * MINIM_BLOCK;  // (below nk, or 0 in the one block of a range without a start)
  B.cnt = B.nk - B.b0 < MINIM_BLOCK ? B.nk - B.b0 : MINIM_BLOCK;
  return B;
}

// sixteen characters of the sequence as four words, character t in byte t & 3 of word t >> 2: pool unit `u` (16-aligned
// offset), of which only the bytes inside [lo, hi) are read; rc: the unit's bytes from the last to the first, complemented
template <bool REV>
__device__ __forceinline__ void minim_unit(const char *__restrict__ pool, long long u, long long lo, long long hi, bool rc, uint32_t x[4]) {
  if (u >= lo && u + 16 <= hi) {
    const uint4 v = *reinterpret_cast<const uint4 *>(pool + u);
    x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
  } else {
    x[0] = x[1] = x[2] = x[3] = 0u;
    for (int b = 0; b < 16; b++) {
      const long long p = u + b;
      if (p >= lo && p < hi) x[b >> 2] |= (uint32_t)(unsigned char)pool[p] << (8 * (b & 3));
    }
  }
  if (REV && rc) {
    const uint32_t a = stats_revcomp4(__builtin_bswap32(x[3])), b = stats_revcomp4(__builtin_bswap32(x[2]));
    const uint32_t c = stats_revcomp4(__builtin_bswap32(x[1])), d = stats_revcomp4(__builtin_bswap32(x[0]));
    x[0] = a, x[1] = b, x[2] = c, x[3] = d;
  } else {
#pragma unroll
    for (int q = 0; q < 4; q++) x[q] &= 0x7F7F7F7Fu;
  }
}

// The roots among the block's starts.  Fills keys[] (LDS of the wavefront) with the keys of [p0, b0 + cnt), p0 = max(0, b0 - w),
// then calls f(j0, valid, root, key) for 64 starts a round, all lanes: the lane's start is j0 + lane (valid: it is one of the block).
template <bool REV, class F>
__device__ __forceinline__ void minim_roots(const sdf_minim_range &R, const MinimBlock &B, const char *__restrict__ pool, int k, int w,
                                            int separate_lowercase, uint32_t *keys, const int lane, F &&f) {
  const bool rc = REV && (R.flags & SDF_MINIM_RC) != 0;
  const long long lo = R.off, hi = R.off + R.len;
  const int p0 = B.b0 > w ? B.b0 - w : 0;
  const int nkeys = B.b0 - p0 + B.cnt;       // keys wanted: those of [p0, b0 + cnt)
  const int nchars = nkeys + k - 1;          // characters wanted: [p0, p0 + nchars)
  // unit 0 is the pool unit that holds character p0; `skip` characters of it lie before p0
  const long long u0 = rc ? (hi - 1 - p0) & ~15ll : (lo + p0) & ~15ll;
  const int skip = rc ? (int)(u0 + 15 - (hi - 1 - p0)) : (int)(lo + p0 - u0);
  const int nunits = (skip + nchars + 15) >> 4;
  const uint32_t kmask = (1u << (2 * k)) - 1u, wmask = (1u << k) - 1u;
  const uint32_t lower = separate_lowercase ? 1u << 30 : 0u;
  for (int m0 = 0; m0 < nunits; m0 += 63) {
    const int m = m0 + lane;
    uint32_t x[4] = {0u, 0u, 0u, 0u};
    if (m < nunits) minim_unit<REV>(pool, rc ? u0 - 16ll * m : u0 + 16ll * m, lo, hi, rc, x);
    uint32_t codes = 0u, flags = 0u;  // flags: bit t: character t is N / n, bit 16 + t: it is an uppercase letter
#pragma unroll
    for (int t = 0; t < 16; t++) {
      const uint32_t c = (x[t >> 2] >> (8 * (t & 3))) & 0xFFu, u = c & 0xDFu;
      const uint32_t code = u == 'C' ? 1u : u == 'G' ? 2u : u == 'T' ? 3u : 0u;
      codes |= code << (30 - 2 * t);
      flags |= (uint32_t)(u == 'N') << t | (uint32_t)(c - 'A' < 26u) << (16 + t);
    }
    const uint32_t codes_next = (uint32_t)__shfl_down((int)codes, 1), flags_next = (uint32_t)__shfl_down((int)flags, 1);
    const uint64_t both = (uint64_t)codes << 32 | codes_next;
    const uint32_t n_bits = (flags & 0xFFFFu) | flags_next << 16, u_bits = flags >> 16 | (flags_next & 0xFFFF0000u);
    if (lane < 63 && m < nunits) {
#pragma unroll
      for (int t = 0; t < 16; t++) {
        const int at = 16 * m + t - skip;  // the start's place among the keys
        const uint32_t hash = (uint32_t)(both >> (64 - 2 * (t + k))) & kmask;
        const uint32_t status = (n_bits >> t) & wmask ? 2u << 30 : (u_bits >> t) & wmask ? 0u : lower;
        if (at >= 0 && at < nkeys) keys[at] = status | hash;
      }
    }
  }
  __syncthreads();  // (the workgroup is this wavefront)
  const int first = B.b0 - p0;  // keys[first] is the key of b0
  for (int jo = 0; jo < B.cnt; jo += 64) {
    const bool valid = jo + lane < B.cnt;
    const int at = valid ? first + jo + lane : first;
    const uint32_t mine = keys[at];
    const int depth = at < w ? at : w;  // (start j has j earlier starts: at == j wherever at < w, because then p0 == 0)
    bool root = valid;
    for (int d = 1; d <= w; d++) {
      if (!__any(root && d <= depth)) break;
      if (d <= depth && keys[at - d] < mine) root = false;
    }
    f(B.b0 + jo, valid, root, mine);
  }
}

// ---- records per block ----
template <bool REV>
__global__ __launch_bounds__(64) void minim_count_kernel(const sdf_minim_range *__restrict__ ranges, int n, const uint64_t *__restrict__ blk0,
                                                         const char *__restrict__ pool, long long pool_bytes, int k, int w,
                                                         int separate_lowercase, uint32_t *__restrict__ counts) {
  __shared__ uint32_t keys[MINIM_BLOCK + MINIM_MAX_W];
  const int lane = threadIdx.x;
  const MinimBlock B = minim_find(ranges, n, blk0, pool_bytes, k, blockIdx.x);
  int cnt = 0;
  if (B.nk > w && B.cnt > 0) {
    cnt = B.b0 == 0 ? 1 : 0;  // the largest root <= w: start 0 is one
    minim_roots<REV>(ranges[B.range], B, pool, k, w, separate_lowercase, keys, lane,
                     [&](int j0, bool valid, bool root, uint32_t) { cnt += __popcll(__ballot(valid && root && j0 + lane > w)); });
  }
  if (lane == 0) counts[blockIdx.x] = (uint32_t)cnt;
}

// ---- first[i] = records of the ranges before i, first[n] = all ----
__global__ __launch_bounds__(256) void minim_first_kernel(const uint64_t *__restrict__ blk0, int n, const uint64_t *__restrict__ block_first,
                                                          uint64_t *__restrict__ first) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i <= n) first[i] = block_first[blk0[i]];
}

// ---- the records.  Nothing is written at or behind out[cap]. ----
template <bool REV>
__global__ __launch_bounds__(64) void minim_emit_kernel(const sdf_minim_range *__restrict__ ranges, int n, const uint64_t *__restrict__ blk0,
                                                        const char *__restrict__ pool, long long pool_bytes, int k, int w,
                                                        int separate_lowercase, const uint64_t *__restrict__ block_first,
                                                        sdf_minimizer *__restrict__ out, uint64_t cap) {
  __shared__ uint32_t keys[MINIM_BLOCK + MINIM_MAX_W];
  const int lane = threadIdx.x;
  const MinimBlock B = minim_find(ranges, n, blk0, pool_bytes, k, blockIdx.x);
  if (B.nk <= w || B.cnt <= 0) return;
  uint64_t at = block_first[blockIdx.x];
  int head = 0;  // (block at start 0) the largest root <= w so far
  auto record = [&](uint32_t key, int loc) {
    sdf_minimizer M;
    M.hash = key & 0x3FFFFFFFu, M.loc = loc, M.status = (int32_t)(key >> 30), M.range = B.range;
    return M;
  };
  if (B.b0 == 0) ++at;
  minim_roots<REV>(ranges[B.range], B, pool, k, w, separate_lowercase, keys, lane, [&](int j0, bool valid, bool root, uint32_t key) {
    const int j = valid ? j0 + lane : j0;
    const unsigned long long early = __ballot(valid && root && j <= w), late = __ballot(valid && root && j > w);
    if (early) head = j0 + 63 - __clzll(early);  // (B.b0 == 0 only; rounds come in ascending order)
    if (valid && root && j > w) {
      const uint64_t idx = at + (uint64_t)__popcll(late & ((1ull << lane) - 1ull));
      if (idx < cap) out[idx] = record(key, j);
    }
    at += (uint64_t)__popcll(late);
  });
  if (B.b0 == 0 && lane == 0) {
    const uint64_t idx = block_first[blockIdx.x];
    if (idx < cap) out[idx] = record(keys[head], head);  // (p0 == 0: keys[j] is start j's)
  }
}

template __global__ void minim_count_kernel<false>(const sdf_minim_range *, int, const uint64_t *, const char *, long long, int, int, int, uint32_t *);
template __global__ void minim_count_kernel<true>(const sdf_minim_range *, int, const uint64_t *, const char *, long long, int, int, int, uint32_t *);
template __global__ void minim_emit_kernel<false>(const sdf_minim_range *, int, const uint64_t *, const char *, long long, int, int, int,
                                                  const uint64_t *, sdf_minimizer *, uint64_t);
template __global__ void minim_emit_kernel<true>(const sdf_minim_range *, int, const uint64_t *, const char *, long long, int, int, int,
                                                 const uint64_t *, sdf_minimizer *, uint64_t);

// ---- the index ----
// sort keys of the records (range << 32 | status << 30 | hash) and their places
__global__ __launch_bounds__(256) void minim_keys_kernel(const sdf_minimizer *__restrict__ recs, long long m, unsigned long long *__restrict__ keys,
                                                         uint32_t *__restrict__ vals) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  const sdf_minimizer M = recs[i];
  keys[i] = (unsigned long long)(uint32_t)M.range << 32 | (unsigned long long)((uint32_t)M.status << 30 | M.hash);
  vals[i] = (uint32_t)i;
}

// the records in sorted order, and a flag on the first record of every group (flags[m] = 0: the scan's total)
__global__ __launch_bounds__(256) void minim_heads_kernel(const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ vals,
                                                          const sdf_minimizer *__restrict__ recs, long long m,
                                                          sdf_minimizer *__restrict__ sorted, uint32_t *__restrict__ flags) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i > m) return;
  if (i == m) {
    flags[i] = 0u;
    return;
  }
  sorted[i] = recs[vals[i]];
  flags[i] = i == 0 || keys[i] != keys[i - 1] ? 1u : 0u;
}

// where every group starts: start[g] for the g-th head, start[groups] = m
__global__ __launch_bounds__(256) void minim_starts_kernel(const uint32_t *__restrict__ flags, const uint32_t *__restrict__ gidx, long long m,
                                                           uint32_t *__restrict__ start) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i > m) return;
  if (i == m || flags[i]) start[gidx[i]] = (uint32_t)i;
}

// a group's sort key: its range, then its size from the largest down
__global__ __launch_bounds__(256) void minim_sizes_kernel(const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ start,
                                                          long long groups, unsigned long long *__restrict__ size_keys) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= groups) return;
  const uint32_t size = start[g + 1] - start[g];
  size_keys[g] = (keys[start[g]] & 0xFFFFFFFF00000000ull) | (0xFFFFFFFFu - size);
}

// Index::Index's walk (src/hash.cc:124-140) for one range per lane.  With the range's group sizes in descending order
// S[0 .. G) and ignore = int(minimizers * 0.001 / 100.0), a size is taken when all groups of that size and of every larger one
// number at most `ignore`: when its last group lies before S[ignore].  The threshold is the smallest size taken -- S[G - 1] when
// G <= ignore, else the last S[t] > S[ignore] with t < ignore --, 2^31 when none is.
__global__ __launch_bounds__(256) void minim_threshold_kernel(const unsigned long long *__restrict__ size_keys, long long groups,
                                                              const uint64_t *__restrict__ first, int n, uint32_t *__restrict__ n_groups,
                                                              uint32_t *__restrict__ threshold) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  auto lower_bound = [&](unsigned long long key) {  // groups with a sort key below `key`
    long long lo = 0, hi = groups;
    while (lo < hi) {
      const long long mid = lo + (hi - lo) / 2;
      if (size_keys[mid] < key) lo = mid + 1;
      else hi = mid;
    }
    return lo;
  };
  const long long g0 = lower_bound((unsigned long long)r << 32), g1 = lower_bound((unsigned long long)(r + 1) << 32);
  const long long G = g1 - g0;
  auto S = [&](long long t) { return 0xFFFFFFFFu - (uint32_t)size_keys[g0 + t]; };
  const long long ignore = (long long)(int)(((double)(first[r + 1] - first[r]) * 0.001) / 100.0);
  uint32_t thr = 0x80000000u;
  if (G > 0 && G <= ignore) {
    thr = S(G - 1);
  } else if (G > 0) {
    const uint32_t pivot = S(ignore);
    long long t = ignore - 1;
    while (t >= 0 && S(t) <= pivot) --t;
    if (t >= 0) thr = S(t);
  }
  n_groups[r] = (uint32_t)G;
  threshold[r] = thr;
}

}  // namespace sdf
