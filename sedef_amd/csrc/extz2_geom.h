// Geometry of the DP kernels: every size, bound and index formula that BOTH a kernel and host code (planner, launcher,
// entry points, traceback) use -- LDS bytes, direction-flag and sync regions, stripe / strip / lane shapes, the limits of
// launch entries.  Plain host + device functions and constants, one definition each; no device-only code in here.
#pragma once
#include "sdf_internal.h"

namespace sdf {

// ---- general kernel (extz2_general.hip) ----
struct BestCell {
  int32_t H, r, key, t;
};
__host__ __device__ inline size_t general_lds_bytes(int qlen, int tlen) {
  const size_t T16 = (size_t)(tlen + 15) / 16 * 16, Q16 = (size_t)(qlen + 15) / 16 * 16;
  return 6 * T16 + Q16 + 16 + 4 * T16 + 16 * sizeof(BestCell) + 16;
}

// ---- wave kernel (extz2_wave.hip) ----
// entries of the LDS sequence windows: the whole (padded) sequence when it is short, else the window slots plus
// 1024 entries of slack (see extz2_pair.hip)
__host__ __device__ inline int wave_tcap(int tlen, int nreg) {
  const int whole = (tlen + 15) / 16 * 16 + 128 * nreg + 32, win = 128 * nreg + 1024 + 64;
  return whole < win ? whole : win;
}
__host__ __device__ inline int wave_qcap(int qlen, int nreg) {
  const int whole = qlen + 128 * nreg + 36, win = 128 * nreg + 1024 + 68;
  return whole < win ? whole : win;
}
// the windows hold the sequences whole?
__host__ __device__ inline bool wave_fits_whole(int qlen, int tlen, int nreg) {
  return wave_tcap(tlen, nreg) == (tlen + 15) / 16 * 16 + 128 * nreg + 32 && wave_qcap(qlen, nreg) == qlen + 128 * nreg + 36;
}
__host__ __device__ inline size_t wave_lds_bytes(int qlen, int tlen, int nreg) {
  return 2 * (size_t)wave_tcap(tlen, nreg) + 2 * (size_t)wave_qcap(qlen, nreg);
}

// ---- pair kernel (extz2_pair.hip) ----
// entries of the LDS sequence windows: the whole (padded) sequence when it is short, else the window slots plus
// 1024 entries of slack (multiples of 4 keep the query window dword aligned behind the target window)
__host__ __device__ inline int pair_tcap(int tlen, int nreg) {
  const int whole = (tlen + 15) / 16 * 16 + 64 * nreg + 32, win = 64 * nreg + 1024 + 64;
  return whole < win ? whole : win;
}
__host__ __device__ inline int pair_qcap(int qlen, int nreg) {
  const int whole = qlen + 64 * nreg + 36, win = 64 * nreg + 1024 + 68;
  return whole < win ? whole : win;
}

// Mixed pairs (round 4): the band schedule of the reference, lo0 = max(0, r - qlen + 1, (r - w + 1) >> 1), hi0 = min(tlen - 1, r,
// (r + w) >> 1) (extern/ksw2_extz2_sse.cc:101-115), depends on the lengths only where the r - qlen + 1 / tlen - 1 clips bite:
// on the last ~w anti-diagonals of a task.  Two tasks of the same (w, flag) but different lengths therefore share every lane
// predicate and every scalar decision up to the first row at which a clip bites for either of them.
// pair_clip_free: the last anti-diagonal r such that on ALL rows 0..r neither clip changes the band of a (qlen, tlen, w)
// task AND the top cell is not yet the target's last column (min(r, (r + w) >> 1) < tlen - 1: the row code tests that too).
__host__ __device__ inline int pair_clip_free(int qlen, int tlen, int w) {
  const int a = 2 * qlen - w - 2;  // r - qlen + 1 <= (r - w + 1) >> 1 for every r up to here (and r - qlen + 1 <= 0 while that is negative)
  const int b = tlen - 2 > 2 * tlen - w - 3 ? tlen - 2 : 2 * tlen - w - 3;  // min(r, (r + w) >> 1) < tlen - 1
  return a < b ? a : b;
}
// rows [0, shared) of two tasks with band w run side by side in one wavefront: a multiple of 16 (the kernel works in
// 16-row blocks), and row `shared` itself is still clip-free for both (a row looks one row ahead for its top cell)
__host__ __device__ inline int pair_shared_rows(int qa, int ta, int qb, int tb, int w) {
  const int ca = pair_clip_free(qa, ta, w), cb = pair_clip_free(qb, tb, w);
  const int c = ca < cb ? ca : cb;
  return c >= 16 ? c / 16 * 16 : 0;
}

constexpr int kMixedMaxNeed = 576;  // widest window of a mixed pair: nine registers of 64 slots (w = 512)
// LDS of a mixed pair: the windows of (max qlen, max tlen) and, behind them, the five state registers of half B per lane
__host__ __device__ inline size_t pair_mixed_lds_bytes(int qmax, int tmax, int nreg) {
  return ((2 * (size_t)pair_tcap(tmax, nreg) + 4 * (size_t)pair_qcap(qmax, nreg) + 15) & ~(size_t)15) + (size_t)5 * nreg * 256;
}
// the windows hold the sequences whole?
__host__ __device__ inline bool pair_fits_whole(int qlen, int tlen, int nreg) {
  return pair_tcap(tlen, nreg) == (tlen + 15) / 16 * 16 + 64 * nreg + 32 && pair_qcap(qlen, nreg) == qlen + 64 * nreg + 36;
}
__host__ __device__ inline size_t pair_lds_bytes(int qlen, int tlen, int nreg) {
  return 2 * (size_t)pair_tcap(tlen, nreg) + 4 * (size_t)pair_qcap(qlen, nreg);
}

// ---- stripe kernel (extz2_stripe.hip) ----
// bytes of LDS of one stripe's wavefront (the reversed query, byte pairs, NSLOT entries of margin either side)
constexpr int kStripeMaxT = 254 * 128;  // widest target: a launch entry has eight bits of stripe index, 255 = idle (sdf_plan.hip)
__host__ __device__ inline size_t stripe_lds_bytes(int qlen, int nreg) {
  return ((size_t)2 * (size_t)(qlen + 256 * nreg) + 15) & ~(size_t)15;
}
// bytes of a task's direction flags (one region per stripe) / of its sync words and edge columns behind them
__host__ __device__ inline size_t stripe_dir_bytes(int qlen, int tlen, int nreg) {
  const int nslot = 128 * nreg, nst = (tlen + nslot - 1) / nslot;
  return (size_t)nst * ((size_t)((qlen + nslot - 1 + 15) / 16) * nreg * 1024);
}
__host__ __device__ inline size_t stripe_sync_bytes(int qlen, int tlen, int nreg) {
  const int nslot = 128 * nreg, nst = (tlen + nslot - 1) / nslot;
  return (((size_t)nst * 8 + 255) & ~(size_t)255) + (size_t)(nst > 1 ? nst - 1 : 0) * (size_t)(qlen + 16) * 4;
}

// The give-up list of the multi-wavefront kernels (stripe_sync.h: stripe_abandon) in the context's misc buffer.
#define SDF_GAVEUP_LIST 32   // (in 64-bit words behind the counter: the list of abandoned tasks, 32-bit entries)
#define SDF_GAVEUP_CAP 65536  // entries of the list (beyond it the batch call fails: "more tasks than can be re-run")
#define SDF_MISC_PARTS (1 + SDF_GAVEUP_LIST + SDF_GAVEUP_CAP / 2)  // (64-bit words of the context's misc buffer before the scan's partial sums)

constexpr size_t kClaimSets = 2048;  // stripe launches per call that take their entries through counters (the rest by index)

// ---- banded stripe kernel (extz2_bstripe.hip) ----
struct BStripeGeom {
  int nslot, nst, blocks_cap, col_len;
  size_t flag_bytes;  // per stripe
};
__host__ __device__ inline BStripeGeom bstripe_geom(int qlen, int tlen, int w, int nreg) {
  BStripeGeom g;
  g.nslot = 128 * nreg;
  const int t16 = (tlen + 15) / 16 * 16;
  g.nst = (t16 + g.nslot - 1) / g.nslot;
  const int rows = 2 * g.nslot + 2 * w < g.nslot + qlen ? 2 * g.nslot + 2 * w : g.nslot + qlen;
  g.blocks_cap = (rows + 32 + 15) / 16 + 2;
  g.col_len = g.blocks_cap * 16 + 64;
  g.flag_bytes = (size_t)g.blocks_cap * nreg * 1024;
  return g;
}
// First / last anti-diagonal of the stripe [T0, T1) (band not cut by its end).  The last one is the last on which it
// has a computed cell; the first one is sixteen columns early: the score refresh runs in 16-cell strides from the band
// START (:124-138), so it reaches up to fifteen cells past the last computed block -- into the first columns of a
// stripe that computes nothing yet, and a cell computed later as part of a widened block may still hold that score.
__host__ __device__ inline int bstripe_first_row(int T0, int w) {
  const int t = T0 >= 16 ? T0 - 16 : 0;
  return t > 2 * t - w ? t : 2 * t - w;
}
__host__ __device__ inline int bstripe_last_row(int T1, int qlen, int tlen, int w) {
  int z = qlen + tlen - 2;
  if (z > T1 + qlen - 2) z = T1 + qlen - 2;
  if (z > 2 * T1 + w - 2) z = 2 * T1 + w - 2;
  return z;
}
// bytes of a task's direction flags / of what lies behind them: a 64-byte record per stripe, then the edge columns
__host__ __device__ inline size_t bstripe_dir_bytes(int qlen, int tlen, int w, int nreg) {
  const BStripeGeom g = bstripe_geom(qlen, tlen, w, nreg);
  return (size_t)g.nst * g.flag_bytes;
}
__host__ __device__ inline size_t bstripe_sync_bytes(int qlen, int tlen, int w, int nreg) {
  const BStripeGeom g = bstripe_geom(qlen, tlen, w, nreg);
  return (size_t)g.nst * 64 + (size_t)(g.nst > 1 ? g.nst - 1 : 0) * (size_t)g.col_len * 8;
}
__host__ __device__ inline size_t bstripe_lds_bytes(int w, int nreg) {
  return ((size_t)2 * (size_t)(6 * 128 * nreg + 2 * w + 256) + 15) & ~(size_t)15;  // reversed-query window, byte pairs
}

// ---- strip kernels (extz2_strip.hip) ----
// columns per lane: 8 (a block of 512 columns per wavefront), or 4 for chains of few wavefronts -- a step of four cells
// is half as long, and a chain of blocks runs at the pace of its steps
constexpr int kStripMaxT = 512;        // widest target of the one-wavefront kernel: one block of 8 columns per lane
constexpr int kStripChainMaxT = 65536;  // ... of a chain of wavefronts, one per block (extz2_strip_chain_kernel): the block index
                                       // of a launch entry has eight bits (256 blocks of 256 columns); the stage's tasks end at 60 kb

__host__ __device__ inline int strip_blocks(int tlen, int cols = 8) { return (tlen + 64 * cols - 1) / (64 * cols); }
__host__ __device__ inline int strip_records(int qlen, int cols) {  // records per block: one per step, or per pair of steps
  return cols == 4 ? (qlen + 64) >> 1 : qlen + 63;
}
__host__ __device__ inline size_t strip_dir_bytes(int qlen, int tlen, int cols = 8, bool solo = false) {
  return (size_t)strip_blocks(tlen, cols) * (size_t)strip_records(qlen, cols) * (solo ? 256 : 512);
}
__host__ __device__ inline size_t strip_lds_bytes(int qlen, int tlen) {
  return strip_blocks(tlen) > 1 ? ((size_t)(qlen + 66) * 4 + 15) & ~(size_t)15 : 16;
}
// chained strips: the edge columns between the blocks of a pair of tasks and, behind them, three words per task of
// partial exact-H values (extz2_strip.hip: "wide targets")
__host__ __device__ inline size_t strip_chain_sync_bytes(int qmax, int tmax, int cols) {
  return ((size_t)(strip_blocks(tmax, cols) - 1) * (size_t)(qmax + 64) * 4 + 64 + 255) & ~(size_t)255;
}

// ---- lane kernel (extz2_lane.hip) ----
constexpr int kLaneMaxLen = 256;      // longest sequence of a lane task
constexpr int kLaneMaxCells = 16384;  // most cells of a lane task: a lane alone on its row costs ~100 cycles per cell

// direction flags of a task: per column tile of 16 target positions one 8-byte record per query position (four 16-bit flag planes: a bit per
// cell), the records of a tile back to back -- a lane writes its region front to back, 8 bytes per row of a tile
__host__ __device__ inline size_t lane_dir_bytes(int qlen, int tlen) { return (size_t)((tlen + 15) >> 4) * (size_t)qlen * 8; }
// launch classes by query length: the LDS of a wavefront is 128 bytes per query position of its longest task
__host__ __device__ inline int lane_class(int qlen) { return qlen <= 32 ? 0 : qlen <= 64 ? 1 : qlen <= 128 ? 2 : 3; }
__host__ __device__ inline size_t lane_lds_bytes(int cls) { return (size_t)128 * (size_t)((32 << cls) + 2); }
// the counting sort of the lane planning (extz2_lane.hip: lane_hist_kernel and on): bits of a key, bins, bins per scan workgroup
constexpr int kLaneKeyBits = 19, kLaneBins = 1 << kLaneKeyBits, kLaneScanBlock = 1024;

// ---- chaining (chain.hip) and alignment statistics (stats_cols.hip) ----
__host__ __device__ inline size_t chain_wave_lds_bytes(int m) {
  if (m <= 0) return 16;
  int bits = 0;
  for (unsigned v = (unsigned)m - 1u; v; v >>= 1) ++bits;
  return (size_t)64 * m + (size_t)16 * ((size_t)2 << bits) + 3 * 48 * 4 + 64;
}

constexpr int STATS_WAVES = 4;  // alignments per workgroup
constexpr uint32_t STATS_GROUP_MAX = 32;  // runs of an alignment that shares its wavefront (SDF_STATS_GROUP_MAX; 0: never)

}  // namespace sdf
