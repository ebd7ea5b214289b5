// Resident sequences: DP tasks that point INTO characters a batch of candidate pairs already has in HBM.
//
// The reference reads the bases of every DP call in place (src/align.cc:49-57: `align_helper` takes two strings the
// caller cut out of the pair's sequences and maps through align_dna, src/align.cc:80-84).  The stage driver uploads a
// super-batch's FASTA characters once, for the seed anchors (anchors.hip); its DP rounds then name their tasks as ranges of
// that pool and this kernel does what `align_dna` + sdf_pack_codes do on the host: characters -> codes (ACGT, either case,
// 0..3; anything else the wildcard 4, src/common.h:60-70,91) -> the packed per-task layout every DP kernel reads
// (include/sedef_hip.h: ceil(len/16) words of 2-bit codes, then ceil(len/32) words of N mask).
#include <hip/hip_runtime.h>

#include "sdf_kernels.h"

namespace sdf {

// Sixteen lanes per sequence (a task is two sequences), a lane per group of 32 bases -- two code words and a mask word.
// SEDEF's tasks are short (708,600 of ~25 bases in a round of the chr1-sized run) with a few of up to 60,000 bases
// (Align::MAX_KSW_SEQ_LEN): the lanes of a group stride over a long sequence.
// REV: some side of some task is reversed.  Such a side is walked from its far end: group g of the task's bases is the 32
// bytes that END at byte len - 32 g of the range, so the sixteen lanes of a step still read 512 contiguous bytes, a lane its
// own 32, as on the forward side; rev_dna (reference: src/common.h:72-77,93) then align_dna give 3 - code for ACGT of either
// case and the wildcard for everything else.
template <bool REV>
__global__ void __launch_bounds__(256) pack_chars_kernel(const PackRec *__restrict__ recs, long long n_seq,
                                                         const char *__restrict__ pool, uint32_t *__restrict__ out) {
  const int sub = threadIdx.x & 15;
  const long long seq = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);
  if (seq >= n_seq) return;
  PackRec r = recs[seq >> 1];
  const bool is_t = (seq & 1) != 0;
  bool rc = false;
  if (REV) {
    rc = ((uint32_t)(is_t ? r.tlen : r.qlen) & kPackRc) != 0;
    r.qlen = (int32_t)((uint32_t)r.qlen & ~kPackRc);
    r.tlen = (int32_t)((uint32_t)r.tlen & ~kPackRc);
  }
  const int len = is_t ? r.tlen : r.qlen;
  const char *src = pool + (is_t ? r.t_byte : r.q_byte);
  const int q_words = ((r.qlen + 15) >> 4) + ((r.qlen + 31) >> 5);
  uint32_t *dst = out + r.q_word + (is_t ? q_words : 0);
  const int ncode = (len + 15) >> 4;
  if (REV && rc) {
    const char *last = src + len - 1;  // base 0 of the reversed side
    for (int g = sub; 32 * g < len; g += 16) {
      uint32_t c0 = 0, c1 = 0, m = 0;
      const int lim = min(32, len - 32 * g);
      for (int b = 0; b < lim; ++b) {
        const unsigned c = (unsigned char)last[-(32 * g + b)] & 0x5fu;
        const unsigned code = c == 'T' ? 0u : c == 'G' ? 1u : c == 'C' ? 2u : c == 'A' ? 3u : 4u;
        if (code == 4u) m |= 1u << b;
        else if (b < 16) c0 |= code << (2 * b);
        else c1 |= code << (2 * (b - 16));
      }
      dst[2 * g] = c0;
      if (32 * g + 16 < len) dst[2 * g + 1] = c1;
      dst[ncode + g] = m;
    }
    return;
  }
  for (int g = sub; 32 * g < len; g += 16) {
    uint32_t c0 = 0, c1 = 0, m = 0;
    const int lim = min(32, len - 32 * g);
    for (int b = 0; b < lim; ++b) {
      const unsigned c = (unsigned char)src[32 * g + b] & 0x5fu;  // (& 127 as the reference's table index, then upper case)
      const unsigned code = c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u;
      if (code == 4u) m |= 1u << b;
      else if (b < 16) c0 |= code << (2 * b);
      else c1 |= code << (2 * (b - 16));
    }
    dst[2 * g] = c0;
    if (32 * g + 16 < len) dst[2 * g + 1] = c1;
    dst[ncode + g] = m;
  }
}

// ---- FASTA layout: a record's sequence lines as they lie in the file -> its bases, back to back, in the resident pool ----
// Base x of the record lies at byte x + (x / line_bases) * (line_bytes - line_bases) of its lines (what a .fai index says;
// reference: src/fasta.cc reads through the same arithmetic), so the gather needs no scan.  `raw` holds whole lines from a line
// start (a piece of the record: sdf_pool_append_fasta streams a long record through a scratch buffer), n bases of them go to
// dst[0..n).  A thread owns one 16-byte-aligned 16-byte slot of the DESTINATION: one vector store; its 16 source bytes
// are contiguous unless a line ends among them (one in four threads at 60 bases a line), then -- and on the ragged first and last
// slot -- it walks byte by byte.  One pass, nothing reused: bound by HBM.
typedef uint32_t u32x4_unaligned __attribute__((ext_vector_type(4), aligned(1)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(256) fasta_gather_kernel(const char *__restrict__ raw, char *__restrict__ dst, uint32_t n,
                                                           uint32_t line_bases, uint32_t gap) {
  const uint32_t head = (uint32_t)((16 - ((uintptr_t)dst & 15)) & 15);  // bases before the first aligned slot
  const long long slot = (long long)blockIdx.x * blockDim.x + threadIdx.x;  // slot 0: the head
  const long long x0l = slot == 0 ? 0 : (long long)head + 16 * (slot - 1);
  if (x0l >= (long long)n) return;
  const uint32_t x0 = (uint32_t)x0l;
  const uint32_t cnt = slot == 0 ? min(head, n) : min(16u, n - x0);
  if (cnt == 0) return;
  const uint32_t line = x0 / line_bases, col = x0 - line * line_bases;
  const char *s = raw + (size_t)x0 + (size_t)line * gap;
  if (cnt == 16 && col + 16 <= line_bases) {
    *(u32x4 *)(dst + x0) = *(const u32x4_unaligned *)s;
    return;
  }
  uint32_t c = col;
  for (uint32_t i = 0; i < cnt; ++i) {
    dst[x0 + i] = *s++;
    if (++c == line_bases) {
      c = 0;
      s += gap;
    }
  }
}

// ---- character classes of ranges of the resident pool (include/sedef_hip.h: sdf_pool_range_classes) ----
// What the stage driver's PairJob asks of every pair: does it hold anything but ACGTNacgtn?  Its table is indexed by the whole
// unsigned char, so a byte of 128 or more is `other` here too -- NOT the class of c & 127, which is what rev_dna and align_dna
// look at.  Four counts per range: ACGT, acgt, N or n, everything else.
//
// A range is cut into segments of kClassSegBytes; a group of sixteen lanes takes one segment and reads the 16-byte ALIGNED slots
// of the pool that hold it, a slot per lane and step: 256 contiguous bytes a step, one vector load a lane.  The bytes of the
// first and the last slot that lie outside the segment are masked, not skipped: no load leaves the slots of the range, and those
// lie inside the pool's allocation (its base is aligned, and it ends 64 bytes or more behind the last character).  Bytes are
// classified four at a time, a flag in bit 7 of each byte of a 32-bit word as in stats_cols.hip.  The group's sums go to the
// range's record with relaxed agent-scope additions, as the lane planner counts its bins; the host zeroes the records in front
// of the launch.
__device__ __forceinline__ void classes_word(uint32_t x, uint32_t valid, int &up, int &lo, int &nn, int &ot) {
  constexpr uint32_t O = 0x01010101u, H = 0x80808080u;
  auto eq = [](uint32_t v, uint32_t c) { return ~((v ^ (c * O)) + 0x7Fu * O) & H; };  // bit 7: byte == c (bytes below 0x80)
  const uint32_t ok = valid & ~x;           // bit 7: a byte of the segment that is below 128
  const uint32_t u = x & (0x5Fu * O);       // bit 7 and the case bit dropped: only 'A' and 'a' become 'A', and so on
  const uint32_t acgt = (eq(u, 'A') | eq(u, 'C') | eq(u, 'G') | eq(u, 'T')) & ok;
  const uint32_t n = eq(u, 'N') & ok;
  const uint32_t lower = x << 2;            // the case bit in bit 7
  up += __popc(acgt & ~lower);
  lo += __popc(acgt & lower);
  nn += __popc(n);
  ot += __popc(valid & ~(acgt | n));
}

__global__ void __launch_bounds__(256) pool_classes_kernel(const ClassRange *__restrict__ ranges, int n_ranges, long long n_seg,
                                                           const char *__restrict__ pool, sdf_range_classes *__restrict__ out) {
  const int sub = threadIdx.x & 15;
  const long long g = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);
  if (g >= n_seg) return;  // (the whole group)
  // the range of segment g: the last one whose seg0 is at most g (ranges without a byte have no segment and share the seg0 of
  // the range behind them)
  int a = 0, b = n_ranges;
  while (b - a > 1) {
    const int mid = (a + b) >> 1;
    if ((long long)ranges[mid].seg0 <= g) a = mid; else b = mid;
  }
  const ClassRange r = ranges[a];
  const long long first = r.off + (g - r.seg0) * (long long)kClassSegBytes;            // the segment: pool bytes [first, last)
  const long long last = min(first + (long long)kClassSegBytes, r.off + (long long)r.len);
  // slots by ADDRESS.  Precondition, checked by the host call: the pool's base is 16-byte aligned, so the slot of the first
  // byte, lo_a & ~15, does not begin below the base; the last slot ends inside the slack behind every pool allocation
  const uintptr_t base = (uintptr_t)pool, lo_a = base + (uintptr_t)first, hi_a = base + (uintptr_t)last;
  int up = 0, lo = 0, nn = 0, ot = 0;
  for (uintptr_t s = (lo_a & ~(uintptr_t)15) + 16u * (unsigned)sub; s < hi_a; s += 256) {
    const u32x4 v = *(const u32x4 *)s;
    if (s >= lo_a && s + 16 <= hi_a) {
      classes_word(v.x, 0x80808080u, up, lo, nn, ot);
      classes_word(v.y, 0x80808080u, up, lo, nn, ot);
      classes_word(v.z, 0x80808080u, up, lo, nn, ot);
      classes_word(v.w, 0x80808080u, up, lo, nn, ot);
    } else {  // the ragged first or last slot (both, in a short range): bit j of m -- byte j of the slot belongs to the segment
      const int j0 = s < lo_a ? (int)(lo_a - s) : 0, j1 = s + 16 > hi_a ? (int)(hi_a - s) : 16;
      const uint32_t m = ((1u << j1) - 1u) & ~((1u << j0) - 1u);
      // (four bits -> bit 7 of four bytes: bit i of the nibble lands on bit 8 i of the product, and on nothing else that is kept)
      auto spread = [](uint32_t nib) { return ((nib * 0x00204081u) & 0x01010101u) << 7; };
      classes_word(v.x, spread(m & 15u), up, lo, nn, ot);
      classes_word(v.y, spread((m >> 4) & 15u), up, lo, nn, ot);
      classes_word(v.z, spread((m >> 8) & 15u), up, lo, nn, ot);
      classes_word(v.w, spread((m >> 12) & 15u), up, lo, nn, ot);
    }
  }
  for (int d = 8; d; d >>= 1) {
    up += __shfl_xor(up, d, 16);
    lo += __shfl_xor(lo, d, 16);
    nn += __shfl_xor(nn, d, 16);
    ot += __shfl_xor(ot, d, 16);
  }
  if (sub == 0) {
    sdf_range_classes *o = out + a;
    if (up) (void)__hip_atomic_fetch_add(&o->upper_acgt, up, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (lo) (void)__hip_atomic_fetch_add(&o->lower_acgt, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (nn) (void)__hip_atomic_fetch_add(&o->n_any, nn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (ot) (void)__hip_atomic_fetch_add(&o->other, ot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---- ranges of the resident pool read back, by strand (include/sedef_hip.h: sdf_pool_fetch_ranges) ----
// dst[dst_off + j] = pool[src_off + j], or rev_dna(pool[src_off + len - 1 - j]) for a reversed range: what the stage driver's
// fetch() does per pair with FastaReference::extract and rc_inplace.  Cut like the counting above: a range's DESTINATION bytes in
// segments of kFetchSegBytes, a group of sixteen lanes per segment.  Source and destination are misaligned independently, so a
// lane works in 16-byte units aligned at the destination: the unit's sixteen source bytes start at any address s, lie in the
// two ALIGNED 16-byte slots of the pool at s & ~15 and behind it, and are cut out of their eight words with word selects and
// funnel shifts; a reversed unit takes the sixteen bytes that END where the forward one would begin to mirror, byte-swaps
// the words in reversed order and maps them four at a time.  Per lane and step: two 16-byte vector loads (the second is the
// first of the lane's neighbour -- same cache line or the next, seven times in eight -- and is not issued at all where source
// and destination are aligned alike), one 16-byte vector store; the sixteen lanes of a group write 256 contiguous bytes a step.
// A slot is loaded only if it is one of the slots of the record's range (those lie inside the pool's allocation: its base is
// aligned, and it ends 64 bytes or more behind the last character); a slot outside reads as zero, and its bytes are never
// among those stored.  The ragged first and last unit of a segment are written byte by byte: a neighbouring range, or the
// neighbouring segment of this one, may own the rest of the unit.  One pass, nothing reused: bound by HBM.

// rev_dna (reference: src/common.h:72-87,93; indexed c & 127) of four characters in one 32-bit word: stats_cols.hip's
// stats_revcomp4, kept as a copy so that the stats kernels' file stays as it is.  A <-> T is ^ 0x15, C <-> G is ^ 0x04, the
// case bit stays; every byte that is not ACGTacgt becomes 'N'.
__host__ __device__ __forceinline__ uint32_t fetch_revcomp4(uint32_t x) {
  constexpr uint32_t O = 0x01010101u, H = 0x80808080u;
  auto ne = [](uint32_t v, uint32_t c) { return (v ^ (c * O)) + 0x7Fu * O; };  // bit 7: byte != c (bytes below 0x80)
  x &= 0x7Fu * O;
  const uint32_t u = x & 0xDFu * O;
  const uint32_t at = ~(ne(u, 'A') & ne(u, 'T')) & H, cg = ~(ne(u, 'C') & ne(u, 'G')) & H;
  const uint32_t flip = (at >> 7) | (at >> 5) | (at >> 3) | (cg >> 5);
  const uint32_t known = at | cg, keep = known | (known - (known >> 7));
  return ((x ^ flip) & keep) | (('N' * O) & ~keep);
}

// (addresses are computed as integers: on the device the accesses are told that they go to global memory, or they would be
// flat ones)
#if defined(__HIP_DEVICE_COMPILE__)
#define SDF_FETCH_GLOBAL __attribute__((address_space(1)))
#else
#define SDF_FETCH_GLOBAL
#endif
// What lane `sub` of the group of segment g does.  Plain C++ for host and device: pool_fetch_kernel is this per lane, and a
// host program can walk the same code over every (g, sub) under a sanitizer.
template <bool REV>
__host__ __device__ __forceinline__ void pool_fetch_lane(const FetchRec *__restrict__ recs, int n_ranges, long long g, int sub,
                                                         const char *__restrict__ pool, char *__restrict__ dst) {
  int a = 0, b = n_ranges;  // the range of segment g: the last one whose seg0 is at most g (pool_classes_kernel)
  while (b - a > 1) {
    const int mid = (a + b) >> 1;
    if ((long long)recs[mid].seg0 <= g) a = mid; else b = mid;
  }
  const FetchRec r = recs[a];
  const long long j0 = (g - (long long)r.seg0) * (long long)kFetchSegBytes;  // the segment: bytes [j0, j1) of the range's output
  const long long j1 = j0 + (long long)kFetchSegBytes < (long long)r.len ? j0 + (long long)kFetchSegBytes : (long long)r.len;
  if (j0 < 0 || j0 >= j1) return;  // (records and n_seg that do not belong together: nothing is touched)
  const uintptr_t d_base = (uintptr_t)dst + (uintptr_t)r.dst_off, d_lo = d_base + (uintptr_t)j0, d_hi = d_base + (uintptr_t)j1;
  const uintptr_t s_lo = (uintptr_t)pool + (uintptr_t)r.src_off, s_hi = s_lo + (uintptr_t)r.len;  // the RANGE's source bytes
  const uintptr_t slot_lo = s_lo & ~(uintptr_t)15, slot_hi = (s_hi + 15) & ~(uintptr_t)15;        // ... and its slots
  const bool rc = REV && r.rc != 0;
  for (uintptr_t u = (d_lo & ~(uintptr_t)15) + 16u * (unsigned)sub; u < d_hi; u += 256) {
    // destination byte u + i comes from source byte s + i (forward), s + 15 - i (reversed); u may lie up to 15 bytes below
    // d_base, and s as far outside [s_lo, s_hi): modulo 2^64, and only the slots of the range are read
    const uintptr_t s = rc ? s_hi - 16 - (u - d_base) : s_lo + (u - d_base);
    const uintptr_t sa = s & ~(uintptr_t)15;
    const unsigned sh = (unsigned)(s & 15);
    u32x4 lo = {0, 0, 0, 0}, hi = {0, 0, 0, 0};
    if (sa >= slot_lo && sa < slot_hi) lo = *(const SDF_FETCH_GLOBAL u32x4 *)sa;
    if (sh != 0 && sa + 16 >= slot_lo && sa + 16 < slot_hi) hi = *(const SDF_FETCH_GLOBAL u32x4 *)(sa + 16);
    // words sh / 4 .. sh / 4 + 4 of the eight, then the bytes from sh % 4 on
    uint32_t w0 = lo.x, w1 = lo.y, w2 = lo.z, w3 = lo.w, w4 = hi.x, w5 = hi.y;
    if (sh & 8) w0 = w2, w1 = w3, w2 = w4, w3 = w5, w4 = hi.z, w5 = hi.w;
    if (sh & 4) w0 = w1, w1 = w2, w2 = w3, w3 = w4, w4 = w5;
    const unsigned bs = (sh & 3) * 8;
    auto funnel = [bs](uint32_t l, uint32_t h) { return (uint32_t)((((uint64_t)h << 32) | l) >> bs); };
    uint32_t o0 = funnel(w0, w1), o1 = funnel(w1, w2), o2 = funnel(w2, w3), o3 = funnel(w3, w4);
    if (rc) {
      const uint32_t t0 = fetch_revcomp4(__builtin_bswap32(o3)), t1 = fetch_revcomp4(__builtin_bswap32(o2));
      const uint32_t t2 = fetch_revcomp4(__builtin_bswap32(o1)), t3 = fetch_revcomp4(__builtin_bswap32(o0));
      o0 = t0, o1 = t1, o2 = t2, o3 = t3;
    }
    if (u >= d_lo && u + 16 <= d_hi) {
      *(SDF_FETCH_GLOBAL u32x4 *)u = u32x4{o0, o1, o2, o3};
    } else {  // the ragged first or last unit of the segment (both, in a short range): bytes [i0, i1) of it are this segment's
      const int i0 = u < d_lo ? (int)(d_lo - u) : 0, i1 = u + 16 > d_hi ? (int)(d_hi - u) : 16;
      const uint32_t o[4] = {o0, o1, o2, o3};
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (i >= i0 && i < i1) ((SDF_FETCH_GLOBAL unsigned char *)u)[i] = (unsigned char)(o[i >> 2] >> (8 * (i & 3)));
    }
  }
}

template <bool REV>
__global__ void __launch_bounds__(256) pool_fetch_kernel(const FetchRec *__restrict__ recs, int n_ranges, long long n_seg,
                                                         const char *__restrict__ pool, char *__restrict__ dst) {
  const long long g = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);
  if (g >= n_seg) return;  // (the whole group)
  pool_fetch_lane<REV>(recs, n_ranges, g, threadIdx.x & 15, pool, dst);
}
#undef SDF_FETCH_GLOBAL

}  // namespace sdf
