// Device helpers the stats kernels share (stats_cols.hip, stats_cuts.hip): sums over the wavefront by DPP, and the eight
// characters of a unit from either strand of a sequence.
#pragma once
#include <hip/hip_runtime.h>

#include "sdf_kernels.h"

namespace sdf {

// Prefix sums and sums over the wavefront (all 64 lanes active): an inclusive scan inside each row of sixteen lanes
// (row_shr 1, 2, 4, 8), the rows' totals passed on (row_bcast 15 into rows 1 and 3, row_bcast 31 into rows 2 and 3) --
// six DPP adds, no LDS; the sum is lane 63's prefix.
__device__ __forceinline__ int stats_wave_scan(int v) {  // inclusive prefix sum over the lanes
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);
  return v;
}
__device__ __forceinline__ int stats_wave_sum(int v) { return __builtin_amdgcn_readlane(stats_wave_scan(v), 63); }

// rev_dna (reference: src/common.h:72-87,93; indexed c & 127) of four characters in one 32-bit word, in the style of
// count_word below: a flag in bit 7 of every byte.  A <-> T is ^ 0x15, C <-> G is ^ 0x04, the case bit stays; every byte that is
// not ACGTacgt becomes 'N'.  All bytes of the result are below 0x80.
__device__ __forceinline__ uint32_t stats_revcomp4(uint32_t x) {
  constexpr uint32_t O = 0x01010101u, H = 0x80808080u;
  auto ne = [](uint32_t v, uint32_t c) { return (v ^ (c * O)) + 0x7Fu * O; };  // bit 7: byte != c (bytes below 0x80)
  x &= 0x7Fu * O;
  const uint32_t u = x & 0xDFu * O;  // (only 'A' and 'a' become 'A', and so on: bit 5 is the case bit of a letter)
  const uint32_t at = ~(ne(u, 'A') & ne(u, 'T')) & H, cg = ~(ne(u, 'C') & ne(u, 'G')) & H;
  const uint32_t flip = (at >> 7) | (at >> 5) | (at >> 3) | (cg >> 5);  // 0x15 / 0x04 in the flagged bytes
  const uint32_t known = at | cg, keep = known | (known - (known >> 7));  // 0xFF in the bytes that are ACGT of either case
  return ((x ^ flip) & keep) | (('N' * O) & ~keep);
}

// Eight consecutive characters of a sequence, as many of them as the sequence still holds (the rest unspecified):
// one unaligned 8-byte load, taken from the last eight bytes of the sequence when fewer remain.
// rc (REV only; per lane): the sequence is the reverse complement of its range.  Its characters pos .. pos + 7 are the eight
// pool bytes that END at slen - pos, last byte first: the same one load, two byte permutes and stats_revcomp4 on either half.
// When fewer than eight remain the load takes the FIRST eight bytes of the range -- no load leaves [s, s + slen) -- and, once
// reversed, the characters wanted are its high ones: the shift of the forward side.
__device__ __forceinline__ uint64_t stats_ld8(const char *p) {
  uint64_t v;
  __builtin_memcpy(&v, p, 8);
  return v;
}
template <bool REV>
__device__ __forceinline__ uint64_t stats_fetch8(const char *s, int pos, int slen, bool wide, bool rc) {
  const int avail = slen - pos;
  if (REV && rc) {
    bool whole = avail >= 8;
    uint64_t v = 0;
    if (wide) {
      v = stats_ld8(s + (whole ? avail - 8 : 0));
      v = (uint64_t)__builtin_amdgcn_perm(0u, (uint32_t)(v >> 32), 0x00010203u) |
          (uint64_t)__builtin_amdgcn_perm(0u, (uint32_t)v, 0x00010203u) << 32;
    } else {
      for (int i = 0; i < avail && i < 8; i++) v |= (uint64_t)(unsigned char)s[avail - 1 - i] << (8 * i);
      whole = true;
    }
    v = (uint64_t)stats_revcomp4((uint32_t)v) | (uint64_t)stats_revcomp4((uint32_t)(v >> 32)) << 32;
    return whole ? v : v >> (8 * (8 - avail));
  }
  if (wide) {  // wave-uniform: the sequence holds eight bytes
    const bool whole = avail >= 8;
    const uint64_t v = stats_ld8(s + (whole ? pos : slen - 8));
    return whole ? v : v >> (8 * (8 - avail));
  }
  uint64_t v = 0;
  for (int i = 0; i < avail && i < 8; i++) v |= (uint64_t)(unsigned char)s[pos + i] << (8 * i);
  return v;
}

constexpr uint64_t STATS_DASHES = 0x2D2D2D2D2D2D2D2DULL;

}  // namespace sdf
