// Coverage of ranges of the resident pool by two interval sets (include/sedef_hip.h: sdf_pool_coverage): `stats diff`.
//
// The reference's get_differences (src/stats_main.cc:397-509) paints the hits of final.bed and of the WGAC table into two
// boost::dynamic_bitset of 250,000,000 bits per chromosome, bit by bit, then walks every base of every chromosome on the host:
// five popcounts of the two bitsets and two counts over the characters.  Here a chromosome is a REGION of the pool, a side of
// a hit an INTERVAL of a region in set 0 (SEDEF) or 1 (WGAC), and three launches do the work, one behind the other on one
// stream:
//   cover_upper_kernel   iv_upper[i] = bytes of interval i with 'A' <= c <= 'Z' (isupper in the C locale: src/stats_main.cc:415-422)
//   cover_paint_kernel   the intervals that are painted (cover_painted: partner < 0, or both counts >= min_upper -- :423) set
//                        their bits
//   cover_count_kernel   per region a, b, both, a_only, b_only, and the bases of the last two with 'A' <= c <= 'Z' && c != 'N'
//                        (:484-497)
// The bitmaps: one bit a base, bit x & 31 of word x >> 5; a region's words start at CoverRegion::word0 -- a word boundary of its
// own, whatever its pool offset --, set 0 in the first `set_words` words of the buffer and set 1 in the second.  The host
// zeroes the buffer and the counters in front of the launches.
//
// An interval is cut into pieces of kCoverPieceBytes; the first two launches give a wavefront to every piece (four to a
// workgroup) and find a piece's interval by CoverIv::piece0, as pool_classes_kernel finds a segment's range: a 100 kb side of a
// hit is thirteen wavefronts, not one.
#include <hip/hip_runtime.h>

#include "sdf_kernels.h"

namespace sdf {

typedef uint32_t cover_u32x4 __attribute__((ext_vector_type(4)));

// bit 7 of every byte of x that is 'A' .. 'Z' (a byte of 128 and above is not); with BASE, and is not 'N'
template <bool BASE>
__device__ __forceinline__ uint32_t cover_flags(const uint32_t x) {
  constexpr uint32_t O = 0x01010101u, H = 0x80808080u;
  const uint32_t y = x & (0x7Fu * O);                // (no sum below carries into the next byte: 0x7F + 0x7F < 0x100)
  const uint32_t ge_a = y + (0x80u - 'A') * O;       // bit 7: y >= 'A'
  const uint32_t gt_z = y + (0x80u - ('Z' + 1)) * O; // bit 7: y > 'Z'
  uint32_t f = ge_a & ~gt_z & ~x & H;
  if (BASE) f &= (y ^ ('N' * O)) + 0x7Fu * O;        // bit 7: y != 'N'
  return f;
}
// bit 7 of the four bytes -> bits 0 .. 3 (bit 8 i of f >> 7 lands on bit 21 + i of the product, and nothing else does)
__device__ __forceinline__ uint32_t cover_nibble(const uint32_t f) { return (((f >> 7) * 0x00204081u) >> 21) & 15u; }

__device__ __forceinline__ int cover_wave_sum(int v) {
  for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// the interval of piece g: the last one whose piece0 is at most g (an interval without a byte has no piece and shares the
// piece0 of the interval behind it)
__device__ __forceinline__ int cover_interval_of(const CoverIv *__restrict__ iv, const int n_iv, const long long g) {
  int a = 0, b = n_iv;
  while (b - a > 1) {
    const int mid = (a + b) >> 1;
    if ((long long)iv[mid].piece0 <= g) a = mid; else b = mid;
  }
  return a;
}

// ---- launch 1: uppercase bytes per interval ----
// A wavefront per piece.  The piece's bytes [first, last) by ADDRESS: up to fifteen bytes in front of the first 16-byte
// boundary, a byte a lane; the aligned slots of sixteen bytes, a vector load a lane and step; the bytes behind the last whole
// slot, a byte a lane.  No load leaves the piece.  One relaxed agent-scope addition per wavefront into the interval's counter.
__global__ void __launch_bounds__(256) cover_upper_kernel(const CoverIv *__restrict__ iv, int n_iv, long long n_pieces,
                                                          const char *__restrict__ pool, int32_t *__restrict__ upper) {
  const int lane = threadIdx.x & 63;
  const long long g = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= n_pieces) return;  // (the whole wavefront)
  const int a = cover_interval_of(iv, n_iv, g);
  const CoverIv r = iv[a];
  const long long lo = (g - r.piece0) * (long long)kCoverPieceBytes;
  const long long hi = min(lo + (long long)kCoverPieceBytes, (long long)r.len);
  const unsigned char *p = (const unsigned char *)pool + r.off + lo;
  const int n = (int)(hi - lo);                                   // 1 .. kCoverPieceBytes
  const int head = min((int)((16u - ((uintptr_t)p & 15u)) & 15u), n);
  const int slots = (n - head) >> 4, tail = (n - head) & 15;
  int up = 0;
  if (lane < head) up += cover_upper(p[lane]);
  const unsigned char *body = p + head;
  for (int s = lane; s < slots; s += 64) {
    const cover_u32x4 v = *(const cover_u32x4 *)(body + 16 * s);
    up += __popc(cover_flags<false>(v.x)) + __popc(cover_flags<false>(v.y)) + __popc(cover_flags<false>(v.z)) +
          __popc(cover_flags<false>(v.w));
  }
  if (lane < tail) up += cover_upper(body[16 * slots + lane]);
  up = cover_wave_sum(up);
  if (lane == 0 && up) (void)__hip_atomic_fetch_add(upper + a, up, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- launch 2: the painted intervals' bits ----
// A wavefront per piece again, a lane per 32-bit word of the piece's bits [lo, hi) and step.  A word the piece covers whole is
// stored as all ones; a word it covers in part -- the first and the last of a piece, so also the word two pieces of one interval
// meet in -- gets its bits by an atomic OR.  Two intervals that touch one word lose nothing: an OR and an OR commute, and a
// store of all ones and an OR end as all ones in either order.
__global__ void __launch_bounds__(256) cover_paint_kernel(const CoverIv *__restrict__ iv, int n_iv, long long n_pieces,
                                                          const int32_t *__restrict__ upper, int32_t min_upper, long long set_words,
                                                          uint32_t *__restrict__ bits) {
  const int lane = threadIdx.x & 63;
  const long long g = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= n_pieces) return;
  const int a = cover_interval_of(iv, n_iv, g);
  const CoverIv r = iv[a];
  if (!cover_painted(r.partner, upper[a], r.partner < 0 ? 0 : upper[r.partner], min_upper)) return;
  const long long off = (g - r.piece0) * (long long)kCoverPieceBytes;
  const long long lo = r.bit0 + off, hi = r.bit0 + min(off + (long long)kCoverPieceBytes, (long long)r.len);  // lo < hi
  const long long w_lo = lo >> 5, w_hi = (hi - 1) >> 5;
  uint32_t *words = bits + (r.set ? set_words : 0);
  for (long long w = w_lo + lane; w <= w_hi; w += 64) {
    uint32_t m = 0xFFFFFFFFu;
    if (w == w_lo) m &= 0xFFFFFFFFu << (unsigned)(lo & 31);
    if (w == w_hi) m &= 0xFFFFFFFFu >> (31u - (unsigned)((hi - 1) & 31));
    if (m == 0xFFFFFFFFu) words[w] = m;
    else (void)__hip_atomic_fetch_or(words + w, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---- launch 3: the seven counts per region ----
// A lane per bitmap word of a region; a region's words in wavefronts of its own (CoverRegion::wave0), so that a wavefront's sums
// belong to one region.  The word's 32 characters start at pool + off + 32 * word, an address of any residue r mod 16 -- the same
// for every word of the region.  They are NOT fetched with narrower loads: the lane reads the aligned 16-byte slots that hold
// them -- two when r == 0, else three --, takes the predicate of all their bytes, four bits a word, and shifts the 48-bit mask
// down by r: the characters are never moved, only their flags.  A slot is read only if it holds a byte of the region, so the
// first slot starts at or behind the pool's base (which is aligned: the host call checks it) and the last one ends within
// fifteen bytes of the region's last character, inside the slack behind every pool allocation; what the ragged slots hold outside
// the region is masked off with the word's valid bits.  A word whose two sets agree on every base needs no character at all.
__global__ void __launch_bounds__(256) cover_count_kernel(const CoverRegion *__restrict__ regions, int n_regions, long long n_waves,
                                                          const char *__restrict__ pool, const uint32_t *__restrict__ bits,
                                                          long long set_words, sdf_cover_counts *__restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long long g = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= n_waves) return;
  int ra = 0, rb = n_regions;
  while (rb - ra > 1) {  // the last region whose wave0 is at most g (cover_interval_of's search)
    const int mid = (ra + rb) >> 1;
    if (regions[mid].wave0 <= g) ra = mid; else rb = mid;
  }
  const CoverRegion R = regions[ra];
  const long long word = (g - R.wave0) * 64 + lane, n_words = ((long long)R.len + 31) >> 5;
  int c_a = 0, c_b = 0, c_both = 0, c_ao = 0, c_bo = 0, c_aou = 0, c_bou = 0;
  if (word < n_words) {
    const long long left = (long long)R.len - 32 * word;  // bases of the region from this word on: >= 1
    const uint32_t valid = left >= 32 ? 0xFFFFFFFFu : (1u << (unsigned)left) - 1u;
    const uint32_t A = bits[R.word0 + word] & valid, B = bits[set_words + R.word0 + word] & valid;
    const uint32_t a_only = A & ~B, b_only = B & ~A;
    c_a = __popc(A), c_b = __popc(B), c_both = __popc(A & B), c_ao = __popc(a_only), c_bo = __popc(b_only);
    if (a_only | b_only) {
      const uintptr_t first = (uintptr_t)pool + (uintptr_t)R.off + (uintptr_t)(32 * word);
      const uintptr_t end = first + (uintptr_t)(left >= 32 ? 32 : left);  // behind the word's last character
      const unsigned r = (unsigned)(first & 15u);
      const uintptr_t slot = first & ~(uintptr_t)15;
      unsigned long long flags = 0;  // bit i: byte i of the slots has upper_base
#pragma unroll
      for (int k = 0; k < 3; k++) {
        if (slot + 16u * k < end) {
          const cover_u32x4 v = *(const cover_u32x4 *)(slot + 16u * k);
          const uint32_t nib = cover_nibble(cover_flags<true>(v.x)) | cover_nibble(cover_flags<true>(v.y)) << 4 |
                               cover_nibble(cover_flags<true>(v.z)) << 8 | cover_nibble(cover_flags<true>(v.w)) << 12;
          flags |= (unsigned long long)nib << (16 * k);
        }
      }
      const uint32_t U = (uint32_t)(flags >> r);
      c_aou = __popc(a_only & U), c_bou = __popc(b_only & U);
    }
  }
  c_a = cover_wave_sum(c_a), c_b = cover_wave_sum(c_b), c_both = cover_wave_sum(c_both), c_ao = cover_wave_sum(c_ao);
  c_bo = cover_wave_sum(c_bo), c_aou = cover_wave_sum(c_aou), c_bou = cover_wave_sum(c_bou);
  if (lane == 0) {
    sdf_cover_counts *o = out + ra;
    const auto add = [](int64_t *p, int v) {
      if (v) (void)__hip_atomic_fetch_add((unsigned long long *)p, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    add(&o->a, c_a), add(&o->b, c_b), add(&o->both, c_both), add(&o->a_only, c_ao), add(&o->b_only, c_bo);
    add(&o->a_only_upper, c_aou), add(&o->b_only_upper, c_bou);
  }
}

}  // namespace sdf
