// Internal types shared by the host C-ABI layer and the gfx950 kernels.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/sedef_hip.h"

namespace sdf {

// [off, off + len) lies inside [0, size) -- an empty range at `size` does -- without ever forming off + len (where that sum
// cannot wrap, a task's 63-bit offset and 31-bit length, this is off + len <= size: what batch_host and batch_pairs asked before)
inline bool in_range(uint64_t off, uint64_t len, uint64_t size) { return off <= size && len <= size - off; }
inline bool in_range(int64_t off, int64_t len, size_t size) { return off >= 0 && len >= 0 && in_range((uint64_t)off, (uint64_t)len, (uint64_t)size); }

// Scoring constants in the form the kernels consume (bytes of the int8 difference domain).
struct ScoreK {
  int32_t q, e;        // gap open / extend as int8 values
  int32_t qe;          // q + e (int)
  uint8_t q_b;         // (uint8)q
  uint8_t qe2_b;       // (uint8)((q+e)*2)
  uint8_t cap_b;       // (uint8)(mat[0] + (q+e)*2)
  uint8_t sc_match;    // (uint8)mat[0]
  uint8_t sc_mis;      // (uint8)mat[1]
  uint8_t wild;        // m-1
  uint8_t pad_[2];
  int8_t mat[25];      // the whole 5x5 matrix: KSW_EZ_GENERIC_SC scores by mat[target * m + query] (reference :139-141)
  int8_t pad2_[3];
};

// The DP kernel the planner gave a task (PlanTask::kind).
enum TaskKind : int32_t {
  kTaskGeneral = 0,     // general kernel (extz2_general.hip), state in LDS; with nreg > 0 the wave kernel (extz2_wave.hip)
  kTaskGeneralHbm = 1,  // general kernel with its state in an HBM slab
  kTaskPair = 2,        // pair kernel (extz2_pair.hip): nreg counts 64-slot registers, the flags are per-task uint2 records
  kTaskPlain = 3,       // general kernel, PLAIN flavour (packed recurrence, H along the band edge only), state in LDS
  kTaskPlainHbm = 4,    // ... state in an HBM slab
  kTaskStripe = 5,      // stripe kernel (extz2_stripe.hip)
  kTaskTrack = 6,       // planning only: the pair kernel's TRACK flavour, made kTaskPair before the launch classes are formed
  kTaskBStripe = 7,     // banded stripe kernel (extz2_bstripe.hip)
  kTaskLane = 8,        // lane kernel (extz2_lane.hip), planned on the device
  kTaskStrip = 9,       // strip kernel (extz2_strip.hip)
  kTaskChain = 10,      // chained strips (extz2_strip.hip)
};

// One planned task as the kernels see it.
struct PlanTask {
  int64_t q_word;    // word offset of the packed query in the pool
  int64_t t_word;    // word offset of the packed target
  int64_t dir_off;   // byte offset of this task's direction matrix in the workspace
  int64_t cig_slot;  // word offset of this task's CIGAR staging slot
  int32_t qlen, tlen;
  int32_t w;         // resolved band (never negative)
  int32_t zdrop;
  int32_t flag;
  int32_t ncol16;    // direction-matrix row stride in cells (n_col_*16 of the reference)
  int32_t out_idx;   // index of the result record
  int32_t cig_cap;   // words in the staging slot
  int32_t nreg;      // 0: general kernel, byte-per-cell direction rows; >0: wave kernel with nreg
                     // packed registers, direction flags in 16-row x 128-slot bit blocks (or what `kind` says)
  TaskKind kind;
};
static_assert(sizeof(PlanTask) == 72 && offsetof(PlanTask, kind) == 68, "PlanTask is uploaded as it is");

// Direction-flag layout of a planned task (traceback.hip: LAYOUT): 0 byte rows, 1 wave-kernel bit blocks, 2 pair-kernel
// records, 3 stripes, 4 banded stripes, 5 lane kernel, 6 strips.
__host__ __device__ inline int dir_layout(const PlanTask &t) {
  return t.nreg == 0 ? 0 : t.kind == kTaskPair ? 2 : t.kind == kTaskStripe ? 3 : t.kind == kTaskBStripe ? 4
         : t.kind == kTaskLane ? 5 : (t.kind == kTaskStrip || t.kind == kTaskChain) ? 6 : 1;
}

// Per-anti-diagonal band geometry (reference: extern/ksw2_extz2_sse.cc:101-115).
struct Band {
  int lo0, hi0;  // logical band [st0, en0]
  int lo, hi;    // widened to whole 16-cell blocks [st, en]
};

__host__ __device__ inline bool band_of(int r, int qlen, int tlen, int w, Band &b) {
  int lo = 0, hi = tlen - 1;
  if (lo < r - qlen + 1) lo = r - qlen + 1;
  if (hi > r) hi = r;
  if (lo < ((r - w + 1) >> 1)) lo = (r - w + 1) >> 1;
  if (hi > ((r + w) >> 1)) hi = (r + w) >> 1;
  b.lo0 = lo;
  b.hi0 = hi;
  b.lo = lo / 16 * 16;            // lo >= 0 whenever lo <= hi
  b.hi = (hi + 16) / 16 * 16 - 1;
  return lo <= hi;
}

}  // namespace sdf
