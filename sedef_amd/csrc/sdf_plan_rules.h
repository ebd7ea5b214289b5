// The planner's per-task rules, each stated once: what a request asks of a kernel, the window a task needs and the
// registers that hold it, the range of tasks each kernel family takes, the launch-order entries and the direction-flag
// bytes of a task of each kind.  cut_batch bounds with them what plan_chunk places with them (sdf_plan.hip).  Host
// only, no device needed.
#pragma once
#include "sdf_batch.h"

namespace sdf {
namespace plan_detail {

// ---- the request ----
// (generic scoring and the approximate-max modes exist in the general kernel only)
constexpr int kGeneralOnlyFlags = SDF_FLAG_RIGHT | SDF_FLAG_EXTZ_ONLY | SDF_FLAG_GENERIC_SC | SDF_FLAG_APPROX_MAX | SDF_FLAG_APPROX_DROP;
// nothing special is asked: only CIGAR / score / mte wanted, no z-drop, no general-only flag, a gap open the kernels take
inline bool simple(const PlanEnv &env, const sdf_task &t) {
  return !(env.want & SDF_WANT_EXT) && t.zdrop < 0 && !(t.flag & kGeneralOnlyFlags) && env.gapo >= 0;
}
// A task that wants no CIGAR needs no direction flags -- except on the stripe kernels, whose progress words,
// hand-over values and edge columns live in HBM right behind the task's flag blocks: those tasks reserve the
// whole layout whatever they want.
inline bool with_dir(const PlanEnv &env, const sdf_task &t) { return env.want_cigar() && !(t.flag & SDF_FLAG_SCORE_ONLY); }
inline uint32_t stage_words(const sdf_task &t) { return (uint32_t)(t.qlen + t.tlen + 2); }  // CIGAR staging words of a task that has any

// ---- band and window ----
inline int resolved_w(const sdf_task &t) { return t.w < 0 ? std::max(t.qlen, t.tlen) : t.w; }
inline bool full_band(const sdf_task &t) { return t.w < 0 || t.w >= std::max(t.qlen, t.tlen); }
inline bool full_band(const PlanTask &p) { return p.w >= std::max(p.qlen, p.tlen); }
inline int ncol16(const sdf_task &t) { return ((std::min(std::min(t.qlen, t.tlen), resolved_w(t) + 1) + 15) / 16 + 1) * 16; }
// window slots: one 16-row block of slack below, the score refresh overshoot above -- but never
// beyond the target's last 16-cell block (cells past it are not part of any window)
inline int window_need(const sdf_task &t) { return std::min(ncol16(t) + 32, (t.tlen + 15) / 16 * 16); }
// the widest window a band allows, whatever the lengths (a mixed pair's other task may have it), at most kMixedMaxNeed
inline int band_window_need(int w) { return std::min(((w + 1 + 15) / 16 + 1) * 16 + 32, kMixedMaxNeed); }
// cells of a row the general kernel passes over (4 per thread and pass: 64, 256 or 1024 threads)
inline int general_width(int ncol16, int tlen) { return std::min(ncol16, (tlen + 15) / 16 * 16); }
// the band reaches the end of both sequences (else it runs out: the traceback starts from the best cell)
inline bool band_whole(const sdf_task &t) {
  const int nrow = t.qlen + t.tlen - 1, w = resolved_w(t);
  Band bl;
  return (w >= 1 || nrow == 1) && band_of(nrow - 1, t.qlen, t.tlen, w, bl);
}

// ---- window need -> registers; 0: beyond the kernel ----
// wave kernel: 1, 2, 3, 4, 6 or 8 registers of 128 slots
inline int wave_nreg(int need) {
  return need <= 128 ? 1 : need <= 256 ? 2 : need <= 384 ? 3 : need <= 512 ? 4 : need <= 768 ? 6 : need <= 1024 ? 8 : 0;
}
// pair kernel, two tasks of one geometry: up to four registers of 64 slots, then 6 and 8
inline int pair_nreg(int need) {
  const int regs = (need + 63) / 64;
  return need > 512 ? 0 : regs <= 4 ? regs : regs <= 6 ? 6 : 8;
}
// pair kernel, MIXED flavour: 2 to 6 registers of 64 slots, then 8 and 9
inline int mixed_nreg(int need) {
  const int regs = (need + 63) / 64;
  return need > kMixedMaxNeed ? 0 : regs <= 2 ? 2 : regs <= 6 ? regs : regs <= 8 ? 8 : 9;
}
// pair kernel, TRACK flavour: rounds its window to 3 / 6 registers of 64 slots
// (wider windows stay on the general kernel: ten registers on one wavefront were measured no faster per row
// than its 1024-thread workgroup, 2.0 vs 1.75 us on 20 kb tasks at w = 512)
inline int track_nreg(int need) { return need <= 192 ? 3 : need <= 384 ? 6 : 0; }

// ---- which tasks a kernel family takes ----
inline bool stripe_range(const PlanEnv &env, const sdf_task &t) { return t.tlen > env.cfg->stripe_min && t.tlen <= kStripeMaxT; }
inline bool stripe_lds_ok(const PlanEnv &env, const sdf_task &t) { return stripe_lds_bytes(t.qlen, 4) <= (size_t)env.max_dyn_lds; }
inline bool strip_range(const sdf_task &t) { return t.tlen > 256 && t.tlen <= kStripMaxT; }           // one wavefront
inline bool chain_range(const sdf_task &t) { return t.tlen > kStripMaxT && t.tlen <= kStripChainMaxT; }  // a chain of them
inline bool strip_rows(const sdf_task &t) { return t.qlen >= 64 && t.qlen < (1 << 18); }
// a superset of what choose_kind gives to the banded stripe kernel (bstripe_wanted): what the cut reserves for
inline bool banded_long(const PlanEnv &env, const sdf_task &t) {
  return env.cfg->bstripe_min_rows > 0 && t.w >= 1 && t.qlen + t.tlen - 1 >= env.cfg->bstripe_min_rows &&
         bstripe_nreg(t.tlen, (int)env.cfg->bstripe_nreg) > 0;
}
// a long banded task, whether its band reaches the end or runs out: the banded stripe kernel (a chain of
// qlen + tlen rows at a hundred instructions each instead of several hundred)
// -- where the one-task kernels are slower per row: windows of more than 192 slots (six or eight registers on
// one wavefront, or the general kernel: 0.9 - 1.9 us per row in a mixed batch against 0.2 - 0.5), and every band
// that runs out (the TRACK flavour: 0.6 us per row with three registers, 1.35 with six; mm8-like mixture with
// those of up to 192 slots left on it 27.5 ms, without 24.1)
inline bool bstripe_wanted(const PlanEnv &env, const sdf_task &t, const bool whole) {
  constexpr int bstripe_plain_min = 192;  // (measured on the mm8-like mixture: 384 -> 47 ms, 192 -> 29-34 ms, 128 -> 36-39 ms)
  const int w = resolved_w(t);
  return simple(env, t) && !env.force_general && env.cfg->bstripe_min_rows > 0 && t.qlen + t.tlen - 1 >= env.cfg->bstripe_min_rows &&
         w >= 1 && !full_band(t) && (env.cfg->bstripe_all /* (tests: every long banded task) */ || window_need(t) > bstripe_plain_min || !whole);
}
// A FEW tasks much longer than the rest of a chunk of chains: a chain's step is ~1 us on blocks of 256 columns, a stripe's row
// 0.25 us, and the launch ends with its longest task -- up to 64 full-band tasks of 12,000 rows + columns and more take the
// stripe kernel next to the chains (the chr1-sized stage run's far-gap round: eight tasks of 8.7 kb a side among 2,500 of
// 1.7 kb: the round's DP 21 -> see profiles/r04_stage.txt).
inline bool long_task(const PlanEnv &env, const sdf_task &t) {
  return t.qlen + t.tlen >= 12000 && stripe_range(env, t) && full_band(t) && stripe_lds_ok(env, t);
}
// a small full-band task with nothing special asked of it is the lane kernel's: sixteen bytes for the device
inline bool lane_task(const sdf_task &t) {
  return t.qlen <= kLaneMaxLen && t.tlen <= kLaneMaxLen && (int64_t)t.qlen * t.tlen <= kLaneMaxCells && full_band(t) && t.zdrop < 0 &&
         !(t.flag & ~(SDF_FLAG_SCORE_ONLY | SDF_FLAG_REV_CIGAR)) && (uint64_t)t.q_off < 0xffffffffull && (uint64_t)t.t_off < 0xffffffffull;
}

// launch-order entries a task may take: a task paired with itself is listed twice, a stripe task once per stripe
// (chained strips take full-band targets of 513..65536 bases whatever stripe_min is: eight idle entries of padding per
// block at most -- ADVICE r3: with SDF_STRIPE_MIN above 512 their launch order overflowed)
inline uint32_t order_entries(const PlanEnv &env, const sdf_task &t) {
  const bool chain = env.strip_ok && chain_range(t);
  return 2 + (stripe_range(env, t) ? (uint32_t)(t.tlen + 127) / 128 : chain ? 8u * (uint32_t)strip_blocks(t.tlen, 4) : 0u) +
         (banded_long(env, t) ? (uint32_t)(t.tlen + 15 + 127) / 128 : 0u);
}

// ---- direction-flag bytes of a task, by the kind that takes it ----
inline size_t round256(size_t x) { return (x + 255) & ~(size_t)255; }
inline size_t row_blocks(int qlen, int tlen) { return (size_t)((qlen + tlen - 1 + 15) / 16); }  // blocks of 16 anti-diagonals
// general kernel: the reference's byte per cell
inline size_t byte_rows_bytes(int qlen, int tlen, int ncol16) { return round256((size_t)(qlen + tlen - 1) * (size_t)ncol16 + 16); }
// wave kernel: 1 KiB per block and register of 128 slots; pair kernels: 512 B per register of 64 slots
inline size_t wave_dir_bytes(int qlen, int tlen, int nreg) { return row_blocks(qlen, tlen) * (size_t)nreg * 1024; }
inline size_t pair_dir_bytes(int qlen, int tlen, int nreg) { return row_blocks(qlen, tlen) * (size_t)nreg * 512; }
// (the stripe kernels keep their inter-stripe words behind the flag blocks: reserved for score-only tasks as well)
inline size_t stripe_region_bytes(int qlen, int tlen, int nreg) {
  return round256(stripe_dir_bytes(qlen, tlen, nreg) + stripe_sync_bytes(qlen, tlen, nreg));
}
inline size_t bstripe_region_bytes(int qlen, int tlen, int w, int nreg) {
  return round256(bstripe_dir_bytes(qlen, tlen, w, nreg) + bstripe_sync_bytes(qlen, tlen, w, nreg));
}
// strip kernels: one flag region per wavefront -- a pair of tasks (or one alone), sized by the taller and the wider;
// chains: the edge columns between the blocks behind the records
inline size_t strip_region_bytes(int qmax, int tmax, int cols, bool alone, bool chain) {
  return round256(strip_dir_bytes(qmax, tmax, cols, alone)) + (chain ? strip_chain_sync_bytes(qmax, tmax, cols) : 0);
}
// What a placed task occupies in its chunk's region (`pb`: its partner, itself when it has none).  A strip / chain pair
// is placed once, with the task of the smaller index (the caller gives the other one 0).
inline size_t placed_dir_bytes(const PlanTask &p, const PlanTask &pb, const bool alone) {
  switch (p.kind) {
    case kTaskStrip: case kTaskChain:
      return strip_region_bytes(std::max(p.qlen, pb.qlen), std::max(p.tlen, pb.tlen), p.nreg, alone, p.kind == kTaskChain);
    case kTaskStripe: return stripe_region_bytes(p.qlen, p.tlen, p.nreg);
    case kTaskBStripe: return bstripe_region_bytes(p.qlen, p.tlen, p.w, p.nreg);
    default: break;
  }
  if (p.flag & SDF_FLAG_SCORE_ONLY) return 0;
  if (p.kind == kTaskPair) return pair_dir_bytes(p.qlen, p.tlen, p.nreg);
  return p.nreg ? wave_dir_bytes(p.qlen, p.tlen, p.nreg) : byte_rows_bytes(p.qlen, p.tlen, p.ncol16);
}

}  // namespace plan_detail
}  // namespace sdf
