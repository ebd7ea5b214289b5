// Every kernel of the library that another file launches, declared once, with the records a kernel takes from the host.
// Each kernel file includes this header, so a definition is checked against its declaration; the launcher and the entry
// points (sdf_launch.hip, sdf_api.hip, sdf_*_api.hip) can only name what is declared here.
#pragma once
#include <hip/hip_runtime.h>

#include "sdf_internal.h"

namespace sdf {

// extz2_general.hip
template <int BS, bool GLOBAL, bool PLAIN>
__global__ void extz2_general_kernel(const PlanTask *, const int32_t *, const uint32_t *, ScoreK, uint8_t *, sdf_result *,
                                     uint8_t *, size_t);
// extz2_wave.hip
template <int NREG, bool STREAM>
__global__ void extz2_wave_kernel(const PlanTask *, const int32_t *, const uint32_t *, ScoreK, uint8_t *, sdf_result *);
// extz2_pair.hip
template <int NREG, bool STREAM, bool TRACK>
__global__ void extz2_pair_kernel(const PlanTask *, const int32_t *, const uint32_t *, ScoreK, uint8_t *, sdf_result *);
template <int NREG>
__global__ void extz2_pair_mixed_kernel(const PlanTask *, const int32_t *, const uint32_t *, ScoreK, uint8_t *,
                                        sdf_result *);
// extz2_stripe.hip
template <int NREG>
__global__ void extz2_stripe_kernel(const PlanTask *, const int32_t *, const uint32_t *, ScoreK, uint8_t *, sdf_result *,
                                    int, unsigned long long *, int, unsigned *);
__global__ void stripe_sync_init_kernel(const PlanTask *, const int32_t *, int, uint8_t *);
// extz2_bstripe.hip
template <int NREG>
__global__ void extz2_bstripe_kernel(const PlanTask *, const int32_t *, const uint32_t *, ScoreK, uint8_t *, sdf_result *,
                                     unsigned long long *, int, unsigned *);
__global__ void bstripe_init_kernel(const PlanTask *, const int32_t *, int, uint8_t *);
__global__ void bstripe_finish_kernel(const PlanTask *, const int32_t *, int, int, const uint8_t *, sdf_result *);
// extz2_lane.hip
struct LaneRec {      // what the host uploads per task of the batch (16 bytes; invalid: flag = 0xffff)
  uint32_t q_word, t_word;  // word offsets of the packed sequences in the pool
  uint32_t out_idx;
  uint8_t qlen_m1, tlen_m1;  // lengths - 1 (1 .. 256)
  uint16_t flag;             // SDF_FLAG_SCORE_ONLY | SDF_FLAG_REV_CIGAR
};
__global__ void lane_keys_kernel(const LaneRec *, int, uint32_t *, uint32_t *);
__global__ void lane_sizes_kernel(const LaneRec *, const uint32_t *, int, unsigned long long *, unsigned long long *);
__global__ void lane_plan_kernel(const LaneRec *, const uint32_t *, int, const unsigned long long *,
                                 const unsigned long long *, int64_t, int64_t, PlanTask *);
__global__ void lane_hist_kernel(const LaneRec *, int, uint32_t *);
__global__ void lane_bins_scan_kernel(const uint32_t *, uint32_t *, unsigned long long *, unsigned long long *, uint32_t *,
                                      unsigned long long *, unsigned long long *);
__global__ void lane_bins_top_kernel(uint32_t *, unsigned long long *, unsigned long long *);
__global__ void lane_place_kernel(const LaneRec *, int, uint32_t *, const uint32_t *, const unsigned long long *,
                                  const unsigned long long *, const uint32_t *, const unsigned long long *,
                                  const unsigned long long *, int64_t, int64_t, PlanTask *);
__global__ void extz2_lane_kernel(const PlanTask *, int, const uint32_t *, ScoreK, uint8_t *, sdf_result *);
// extz2_strip.hip
__global__ void extz2_strip_kernel(const PlanTask *, const int32_t *, const uint32_t *, ScoreK, uint8_t *, sdf_result *);
template <int C>
__global__ void extz2_strip_chain_kernel(const PlanTask *, const int32_t *, const uint32_t *, ScoreK, uint8_t *,
                                         sdf_result *, unsigned long long *, int, unsigned *);
__global__ void strip_chain_init_kernel(const PlanTask *, const int32_t *, uint8_t *);
// traceback.hip
template <int LAYOUT, int G>
__global__ void traceback_kernel(const PlanTask *, int, const uint32_t *, const uint8_t *, sdf_result *, uint32_t *);
__global__ void cigar_scan_blocks_kernel(sdf_result *, int, unsigned long long *);
__global__ void cigar_scan_parts_kernel(unsigned long long *, int, unsigned long long *);
__global__ void cigar_scan_add_kernel(sdf_result *, int, const unsigned long long *);
__global__ void cigar_compact_kernel(const PlanTask *, int, const sdf_result *, const uint32_t *, uint32_t *,
                                     unsigned long long);
// sdf_launch.hip
__global__ void reset_results_kernel(sdf_result *res, int n);
// seq_pack.hip
struct PackRec {     // one DP task's two character ranges and where its packed words go (32 bytes)
  int64_t q_byte;    // first character of the query range in the pool (the first byte in pool order, whatever the strand)
  int64_t t_byte;
  int64_t q_word;    // first packed word of the query; the target's words follow the query's
  int32_t qlen, tlen;  // bit 31 (kPackRc): the side is read reverse-complemented -- base i = rev(pool[byte + len - 1 - i])
};
// The two strand bits of a task (SDF_TASK_Q_RC / SDF_TASK_T_RC) travel in the sign bits of the lengths, which are never
// negative: the record stays 32 bytes.  Only pack_chars_kernel<true> decodes them; a batch without a reversed side is
// packed by pack_chars_kernel<false>, the kernel as it was.
constexpr uint32_t kPackRc = 0x80000000u;
static_assert(sizeof(PackRec) == 32, "PackRec: two records per 64-byte line");
template <bool REV>
__global__ void pack_chars_kernel(const PackRec *, long long, const char *, uint32_t *);
__global__ void fasta_gather_kernel(const char *, char *, uint32_t, uint32_t, uint32_t);
struct ClassRange {  // one range of sdf_pool_range_classes (16 bytes)
  int64_t off;       // first byte of the range in the pool
  int32_t len;
  int32_t seg0;      // segments of the ranges before this one: the launch's group g counts segment g - seg0 of its range
};
constexpr int kClassSegBytes = 16384;  // bytes of a range that one group of sixteen lanes counts
static_assert(sizeof(ClassRange) == 16 && sizeof(sdf_range_classes) == 16, "four records per 64-byte line");
__global__ void pool_classes_kernel(const ClassRange *, int, long long, const char *, sdf_range_classes *);
// one range of sdf_pool_fetch_ranges (include/sedef_hip.h: sdf_pool_fetch_rec, 32 bytes): len bytes from pool + src_off to
// dst + dst_off, reversed and complemented when rc; seg0 as ClassRange has it
using FetchRec = sdf_pool_fetch_rec;
constexpr int kFetchSegBytes = SDF_FETCH_SEG_BYTES;  // destination bytes of a range that one group of sixteen lanes writes
static_assert(sizeof(FetchRec) == 32, "FetchRec: two records per 64-byte line");
// REV: some record of the launch has rc set; <false> never reads the word and is the plain copy
template <bool REV>
__global__ void pool_fetch_kernel(const FetchRec *, int, long long, const char *, char *);
// pool_cover.hip
constexpr int kCoverPieceBytes = 8192;  // bytes (and bitmap bits) of an interval that one wavefront counts or paints
struct CoverRegion {  // one region of sdf_pool_coverage (32 bytes)
  int64_t off;        // first byte of the region in the pool
  int64_t word0;      // first word of the region's bitmap within a set's half of the buffer: the words of the regions before it
  int64_t wave0;      // wavefronts of the count launch before this region's: ceil(words / 64) each
  int32_t len, pad;
};
struct CoverIv {    // one interval (32 bytes)
  int64_t off;      // first byte of the interval in the pool
  int64_t bit0;     // its first bit within a set's half of the buffer: 32 * word0 of its region + start
  int32_t len, set, partner;
  int32_t piece0;   // pieces of the intervals before this one: the launch's wavefront g takes piece g - piece0 of its interval
};
static_assert(sizeof(CoverRegion) == 32 && sizeof(CoverIv) == 32 && sizeof(sdf_cover_counts) == 56 && sizeof(sdf_cover_interval) == 24,
              "include/sedef_hip.h");
// the two predicates of include/sedef_hip.h on one byte, and the rule of the paint launch: the one form the kernels' word forms
// are checked against and the host form uses
__host__ __device__ inline bool cover_upper(const unsigned char c) { return c >= 'A' && c <= 'Z'; }
__host__ __device__ inline bool cover_upper_base(const unsigned char c) { return c >= 'A' && c <= 'Z' && c != 'N'; }
__host__ __device__ inline bool cover_painted(const int32_t partner, const int32_t own, const int32_t partners, const int32_t min_upper) {
  return partner < 0 || (own >= min_upper && partners >= min_upper);
}
__global__ void cover_upper_kernel(const CoverIv *, int, long long, const char *, int32_t *);
__global__ void cover_paint_kernel(const CoverIv *, int, long long, const int32_t *, int32_t, long long, uint32_t *);
__global__ void cover_count_kernel(const CoverRegion *, int, long long, const char *, const uint32_t *, long long, sdf_cover_counts *);
// bucket_merge.hip
struct BucketRec {  // a seed hit behind steps 1 and 2 of include/sedef_hip.h (sdf_bucket_merge): extended, sides ordered (32 bytes)
  int32_t q_chr, q_start, q_end, r_chr, r_start, r_end;
  uint32_t flags;  // SDF_SEED_RC | kBucketSelf | kBucketBad
  int32_t pair;    // group_pair_order of the two chromosomes' groups
};
struct BucketBox {  // a window of the sweep (16 bytes)
  int32_t q_start, q_end, r_start, r_end;
};
struct BucketSeg {  // an item of the segmented max-scan: head of a segment, largest q_end so far
  int32_t head, val;
};
struct BucketSegMax {
  __host__ __device__ BucketSeg operator()(const BucketSeg &a, const BucketSeg &b) const {
    return b.head ? b : BucketSeg{a.head, a.val > b.val ? a.val : b.val};
  }
};
static_assert(sizeof(BucketRec) == 32 && sizeof(sdf_seed_hit) == 32 && sizeof(sdf_bucket_hit) == 32 && sizeof(sdf_bucket_params) == 24,
              "include/sedef_hip.h");
constexpr uint32_t kBucketSelf = 2;  // a region against itself: takes no part in the sweep
constexpr uint32_t kBucketBad = 4;   // fails a check of include/sedef_hip.h (the device form drops and counts it)
constexpr uint32_t kBucketDeadClass = 1u << 22;  // sort key of a slot that does not leave; above every class (2^31 / 1000 < 2^22)
// The checks of one record and steps 1 and 2, the one form the kernel and the host forms share.  A record that fails a check
// comes back as kBucketBad with nothing else defined.
__host__ __device__ inline BucketRec bucket_prepare(const sdf_seed_hit &h, const int32_t *chr_group, const int32_t n_chr,
                                                    const int32_t *group_pair_order, const int32_t n_groups, const double extend_ratio,
                                                    const int32_t max_extend, const int32_t merge_dist) {
#pragma clang fp contract(off)
  BucketRec r{h.q_chr, h.q_start, h.q_end, h.r_chr, h.r_start, h.r_end, h.flags, 0};
  const int64_t top = (int64_t)0x7fffffff - max_extend - merge_dist;
  bool ok = (h.flags & ~SDF_SEED_RC) == 0 && h.pad == 0 && h.q_chr >= 0 && h.q_chr < n_chr && h.r_chr >= 0 && h.r_chr < n_chr;
  ok = ok && h.q_start >= 0 && h.r_start >= 0 && h.q_start <= h.q_end && h.r_start <= h.r_end && h.q_end <= top && h.r_end <= top;
  int32_t w = ok ? (h.q_end - h.q_start > h.r_end - h.r_start ? h.q_end - h.q_start : h.r_end - h.r_start) : 0;
  const double grown = extend_ratio * w;
  ok = ok && grown < 2147483648.0;
  int32_t gq = 0, gr = 0;
  if (ok) {
    gq = chr_group[h.q_chr], gr = chr_group[h.r_chr];
    ok = gq >= 0 && gq < n_groups && gr >= 0 && gr < n_groups;
  }
  if (!ok) return r.flags = kBucketBad, r;
  w = (int32_t)grown;  // Hit::extend, operation by operation
  w = max_extend < w ? max_extend : w;
  r.q_start = r.q_start - w > 0 ? r.q_start - w : 0;
  r.q_end += w;
  r.r_start = r.r_start - w > 0 ? r.r_start - w : 0;
  r.r_end += w;
  // order_sides: std::tie(name, start, end) of the query > that of the reference
  const bool swap = r.q_chr != r.r_chr ? r.q_chr > r.r_chr : r.q_start != r.r_start ? r.q_start > r.r_start : r.q_end > r.r_end;
  if (swap) {
    int32_t t;
    t = r.q_chr, r.q_chr = r.r_chr, r.r_chr = t;
    t = r.q_start, r.q_start = r.r_start, r.r_start = t;
    t = r.q_end, r.q_end = r.r_end, r.r_end = t;
    t = gq, gq = gr, gr = t;
  }
  r.pair = group_pair_order[(int64_t)gq * n_groups + gr];
  if (r.pair < 0 || r.pair >= n_groups * n_groups) return r.flags = kBucketBad, r;
  if (r.q_chr == r.r_chr && r.q_start == r.r_start && r.q_end == r.r_end && !(r.flags & SDF_SEED_RC)) r.flags |= kBucketSelf;
  return r;
}
// the two sort keys of a prepared record: key_hi first, key_lo among equals
__host__ __device__ inline uint64_t bucket_key_hi(const BucketRec &r) {
  return (uint64_t)r.pair << 39 | (uint64_t)(r.flags & SDF_SEED_RC) << 38 | (uint64_t)r.q_chr << 19 | (uint64_t)r.r_chr;
}
__host__ __device__ inline uint64_t bucket_key_lo(const BucketRec &r) { return (uint64_t)r.q_start << 32 | (uint32_t)r.r_start; }
// merge()'s test of a window against the growing hit (src/merge.cc:73-76 with its lower_bound: the second clause)
__host__ __device__ inline bool bucket_apart(const BucketBox &w, const BucketBox &h, const int32_t merge_dist) {
  return w.q_end + merge_dist < h.q_start || w.r_end < h.r_start - merge_dist || w.r_start > h.r_end + merge_dist;
}
// the complexity class of a merged hit (src/align_main.cc:128-130): a correctly rounded product and root on both sides
__host__ __device__ inline int32_t bucket_class(const BucketBox &b) {
#pragma clang fp contract(off)
  const double area = (double)(b.q_end - b.q_start) * (double)(b.r_end - b.r_start);
#ifdef __HIP_DEVICE_COMPILE__
  return (int32_t)__dsqrt_rn(area) / 1000;
#else
  return (int32_t)__builtin_sqrt(area) / 1000;
#endif
}
__global__ void bucket_prepare_kernel(const sdf_seed_hit *, int, const int32_t *, int, const int32_t *, int, double, int, int, BucketRec *,
                                      unsigned long long *, unsigned long long *, uint32_t *, unsigned long long *);
__global__ void bucket_key_gather_kernel(const unsigned long long *, const uint32_t *, int, unsigned long long *);
__global__ void bucket_runs_kernel(const BucketRec *, const uint32_t *, const unsigned long long *, int, BucketRec *, BucketSeg *);
__global__ void bucket_new_run_kernel(const BucketRec *, const BucketSeg *, int, int, uint32_t *, BucketBox *, uint32_t *);
__global__ void bucket_run_starts_kernel(const uint32_t *, const uint32_t *, int, uint32_t *);
__global__ void bucket_sweep_kernel(BucketBox *, uint32_t *, const uint32_t *, const uint32_t *, int);
__global__ void bucket_flush_keys_kernel(const BucketBox *, const uint32_t *, const uint32_t *, const uint32_t *, int,
                                         unsigned long long *, uint32_t *);
__global__ void bucket_class_kernel(const unsigned long long *, const uint32_t *, const BucketRec *, const BucketBox *, int,
                                    sdf_bucket_hit *, uint32_t *, uint32_t *, unsigned long long *);
__global__ void bucket_deal_kernel(const uint32_t *, const uint32_t *, int, int, sdf_bucket_hit *);
// seed_records.hip
static_assert(sizeof(sdf_seed_job) == 24 && sizeof(sdf_search_pair_hit) == 24, "include/sedef_hip.h");
// The job of hit t: the last j in [0, n_jobs) with first[j] <= t (n_jobs >= 1).  Jobs without hits repeat a value of first[] and
// are stepped over; whatever first[] holds, the answer is inside the job table.
__host__ __device__ inline size_t seed_job_of(const uint64_t *first, const size_t n_jobs, const uint64_t t) {
  size_t lo = 0, hi = n_jobs;  // (the answer is in [lo, hi))
  while (hi - lo > 1) {
    const size_t mid = lo + (hi - lo) / 2;
    if (first[mid] <= t) lo = mid;
    else hi = mid;
  }
  return lo;
}
// The record of a hit of job `job` (include/sedef_hip.h: sdf_seed_records), the one form the kernel and the host form share: the
// flip of search_hit_bed in the low 32 bits of its size_t arithmetic.
__host__ __device__ inline sdf_seed_hit seed_record(const sdf_search_pair_hit &h, const sdf_seed_job &job) {
  const bool rc = (job.flags & SDF_SEED_RC) != 0;
  const uint32_t len = (uint32_t)(uint64_t)job.ref_len;
  const int32_t r_start = rc ? (int32_t)(len - (uint32_t)h.ref_end + 1u) : h.ref_start;
  const int32_t r_end = rc ? (int32_t)(len - (uint32_t)h.ref_start + 1u) : h.ref_end;
  return sdf_seed_hit{job.q_chr, h.query_start, h.query_end, job.r_chr, r_start, r_end, rc ? SDF_SEED_RC : 0u, 0u};
}
__global__ void seed_records_kernel(const sdf_search_pair_hit *, uint32_t, const uint64_t *, const sdf_seed_job *, size_t, sdf_seed_hit *);
// anchors.hip
struct AnchorPairDev {
  int64_t q_off, r_off;    // byte offsets of the raw sequences in the pool
  int32_t qlen, rlen;
  int32_t same_chr, delta;  // near-diagonal filter of self comparisons (:67-69); same_chr: kPairSameChr | kPairRefRc
  int64_t rk_start, qk_start;  // first global k-mer index of this pair's reference / query
};
// AnchorPairDev::same_chr holds two truth values (sdf_anchor_pair::same_chr is one, and stays one)
constexpr int32_t kPairSameChr = 1;
constexpr int32_t kPairRefRc = 2;  // the reference range is read reverse-complemented (sdf_anchors_batch_strand: r_rc)
struct CandOut {
  int32_t q, r, l, has_u;
};
template <bool RC>
__global__ void ref_keys_kernel(const AnchorPairDev *, int, const char *, int, int, unsigned long long *);
__global__ void query_lookup_kernel(const AnchorPairDev *, int, const char *, int, int, const unsigned long long *,
                                    long long, uint32_t *, uint32_t *, uint32_t *, uint32_t *);
template <bool RC>
__global__ void candidates_kernel(const AnchorPairDev *, const char *, int, const unsigned long long *, const uint32_t *,
                                  const uint32_t *, const unsigned long long *, const uint32_t *, long long, long long,
                                  uint32_t *, CandOut *, int);
__global__ void anchors_compact_kernel(const uint32_t *, const unsigned long long *, const CandOut *, long long, CandOut *,
                                       unsigned long long);
__global__ void anchor_offsets_kernel(const AnchorPairDev *, int, const unsigned long long *, const unsigned long long *,
                                      long long, unsigned long long, long long, long long *);
// chain.hip
__global__ void chain_kernel(const sdf_anchor *, const int64_t *, const int64_t *, int, int, int, int32_t *, int32_t *,
                             int32_t *, int32_t *, const int32_t *);
__global__ void chain_wave_kernel(const sdf_anchor *, const int64_t *, const int32_t *, int, int, int32_t *, int32_t *,
                                  int32_t *);
__global__ void chain_tree_script_kernel(const int32_t *, int, const int32_t *, int, int32_t *, int, int32_t *, int32_t *);
// stats_cols.hip
struct StatsItem {  // a segment of a long alignment
  sdf_stats_task t;
  uint32_t task;  // the alignment it belongs to (0xffffffff: nothing to do)
  uint32_t pad;
};
// REV: some task of the launch carries SDF_STATS_A_RC / SDF_STATS_B_RC in `reserved`; <false> never reads the word
template <bool REV>
__global__ void stats_columns_kernel(const sdf_stats_task *, int, const char *, const uint32_t *, sdf_stats_cols *,
                                     StatsItem *, unsigned *, unsigned, unsigned);
template <bool REV>
__global__ void stats_segments_kernel(const StatsItem *, const unsigned *, unsigned, const char *, const uint32_t *,
                                      sdf_stats_cols *);
// stats_cuts.hip
struct CutsScores {  // the trims' column scores (host: Params::match and on)
  int match, mismatch, gap_open, gap_extend;
};
// an alignment's word of the count launch: pieces, and two flags
constexpr uint32_t kCutsEvents = 0x80000000u, kCutsBad = 0x40000000u, kCutsCount = 0x3fffffffu;
template <bool REV>
__global__ void stats_cuts_count_kernel(const sdf_stats_task *, int, const char *, const uint32_t *, uint32_t *, int32_t *);
__global__ void stats_cuts_scan_kernel(const uint32_t *, int, uint64_t *);
template <bool REV>
__global__ void stats_cuts_emit_kernel(const sdf_stats_task *, int, const char *, const uint32_t *, CutsScores, const uint32_t *,
                                       const int32_t *, const uint64_t *, sdf_stats_piece *, uint64_t);
// minimizers.hip
constexpr int MINIM_BLOCK = SDF_MINIM_BLOCK;  // k-mer starts of one range that one wavefront takes
constexpr int MINIM_MAX_W = SDF_MINIM_MAX_W;  // (a wavefront's LDS holds the keys of MINIM_BLOCK + MINIM_MAX_W starts; MINIM_BLOCK > MINIM_MAX_W:
                                              // the block at start 0 sees every root <= w)
static_assert(MINIM_BLOCK > MINIM_MAX_W && MINIM_BLOCK % 64 == 0, "minimizers.hip: the first block holds the starts 0 .. w");
static_assert(sizeof(sdf_minim_range) == 16 && sizeof(sdf_minimizer) == 16, "four records per 64-byte line");
__global__ void minim_blocks_kernel(const sdf_minim_range *, int, long long, int, uint32_t *);
// REV: some range of the launch carries SDF_MINIM_RC; <false> never reads the word
template <bool REV>
__global__ void minim_count_kernel(const sdf_minim_range *, int, const uint64_t *, const char *, long long, int, int, int, uint32_t *);
__global__ void minim_first_kernel(const uint64_t *, int, const uint64_t *, uint64_t *);
template <bool REV>
__global__ void minim_emit_kernel(const sdf_minim_range *, int, const uint64_t *, const char *, long long, int, int, int,
                                  const uint64_t *, sdf_minimizer *, uint64_t);
__global__ void minim_keys_kernel(const sdf_minimizer *, long long, unsigned long long *, uint32_t *);
__global__ void minim_heads_kernel(const unsigned long long *, const uint32_t *, const sdf_minimizer *, long long, sdf_minimizer *,
                                   uint32_t *);
__global__ void minim_starts_kernel(const uint32_t *, const uint32_t *, long long, uint32_t *);
__global__ void minim_sizes_kernel(const unsigned long long *, const uint32_t *, long long, unsigned long long *);
__global__ void minim_threshold_kernel(const unsigned long long *, long long, const uint64_t *, int, uint32_t *, uint32_t *);
// search_seeds.hip
constexpr int SEARCH_MAX_MEMBERS = SDF_SEARCH_MAX_MEMBERS, SEARCH_MAX_GATHER = SDF_SEARCH_MAX_GATHER;  // a wavefront's LDS: 16-bit offsets, 32-bit positions
static_assert(SEARCH_MAX_GATHER < 65535 && (SEARCH_MAX_GATHER & (SEARCH_MAX_GATHER - 1)) == 0, "search_seeds.hip: offsets are 16 bits wide");
struct SearchLook {       // what search_lookup_kernel and search_prev_kernel leave per query minimizer j (16 bytes)
  uint32_t start, size;   // j's group in r_sorted; size 0: j does not seed, or the group is absent or at / over the threshold
  int32_t prev;           // the last minimizer before j with j's (status, hash), -1: none
  int32_t end;            // the members of window j are [j, end)
};
static_assert(sizeof(SearchLook) == 16 && sizeof(sdf_search_window) == 20 && sizeof(sdf_search_interval) == 8, "include/sedef_hip.h");
__global__ void search_keys_kernel(const sdf_minimizer *, int, unsigned long long *, uint32_t *);
__global__ void search_prev_kernel(const unsigned long long *, const uint32_t *, int, SearchLook *);
__global__ void search_lookup_kernel(const sdf_minimizer *, int, const sdf_minimizer *, int, uint32_t, int, int, SearchLook *);
// search_found.hip: the bin index over the query axis of the found records, as the kernels that read it take it
constexpr int FOUND_MAX = SDF_SEARCH_MAX_FOUND, FOUND_BIN_SHIFT = SDF_SEARCH_FOUND_BIN_SHIFT;
constexpr int FOUND_BINS = 1 << (31 - FOUND_BIN_SHIFT);  // every base a 32-bit loc can name; a base below 0 counts as 0
static_assert(sizeof(sdf_search_found) == 16, "include/sedef_hip.h");
struct FoundIndex {
  const sdf_search_found *found;
  const unsigned long long *start;  // FOUND_BINS + 1: bin b's entries are entries[start[b], start[b + 1])
  const uint32_t *entries;          // record ids; none at or behind entries[cap]
  const uint32_t *visible;          // a prefix length per window (search_window_kernel) or per interval (search_overlap_kernel)
  unsigned long long cap;
  uint32_t nf;
};
__host__ __device__ inline int found_bin(const long long base) {
  return base < 0 ? 0 : base > 0x7fffffffll ? FOUND_BINS - 1 : (int)(base >> FOUND_BIN_SHIFT);
}
__host__ __device__ inline bool found_empty(const sdf_search_found &R) { return R.q_start >= R.q_end || R.r_start >= R.r_end; }
__host__ __device__ inline bool found_covers(const sdf_search_found &R, const long long loc, const long long pos) {
  return R.q_start <= loc && loc < R.q_end && R.r_start <= pos && pos < R.r_end;
}
// a record that can contain the loc of a member of the window at qs: the ones SDF_SEARCH_FOUND_WIDE counts
__host__ __device__ inline bool found_meets_window(const sdf_search_found &R, const long long qs, const long long init_len) {
  return !found_empty(R) && R.q_start <= qs + init_len && R.q_end > qs;
}
// is_overlap's answer on ONE record that covers (pf_pos, pfp_pos): rules 2 to 4 of include/sedef_hip.h; the one form the
// kernel and the host form share
__host__ __device__ inline bool found_overlaps(const sdf_search_found &R, const long long pf_pos, const long long pf_end,
                                               const long long pfp_pos, const long long pfp_end, const int min_read_size) {
  const long long sA = R.q_start, eA = R.q_end, sB = R.r_start, eB = R.r_end;
  if (pf_pos >= sA && pf_end <= eA && pfp_pos >= sB && pfp_end <= eB) return true;
  const long long small = eA - sA < eB - sB ? eA - sA : eB - sB;
  if ((double)small < min_read_size * 1.5) return false;
  return eA - pf_pos >= min_read_size && eB - pfp_pos >= min_read_size;
}
__global__ void found_count_kernel(const sdf_search_found *, int, unsigned long long *);
__global__ void found_fill_kernel(const sdf_search_found *, int, const unsigned long long *, unsigned long long *, uint32_t *,
                                  unsigned long long, unsigned long long *);
__global__ void search_overlap_kernel(const sdf_minimizer *, int, const uint64_t *, const sdf_search_roll_rec *, int, FoundIndex, int, int,
                                      uint32_t *, sdf_filter_task *);
// EMIT false: the windows' records and interval counts; true: the intervals.  FOUND: with the exclusions of the found records
// (the index is read by these instantiations alone)
template <bool EMIT, bool FOUND>
__global__ void search_window_kernel(const sdf_minimizer *, int, long long, const sdf_minimizer *, const SearchLook *, int, int,
                                     const int32_t *, int, sdf_search_window *, uint32_t *, const uint64_t *, sdf_search_interval *,
                                     uint64_t, FoundIndex);
// search_seeds_wide.hip: a workgroup of SEARCH_WIDE_THREADS lanes per window that search_window_kernel flags and leaves; its
// LDS: 32-bit keys of SEARCH_WIDE_MAX_GATHER positions, 32-bit offsets of the members, a chunk of SEARCH_WIDE_CHUNK found records
constexpr int SEARCH_WIDE_MAX_GATHER = SDF_SEARCH_WIDE_MAX_GATHER, SEARCH_WIDE_THREADS = 256, SEARCH_WIDE_CHUNK = 256;
constexpr size_t SEARCH_WIDE_MAX_LIST = (size_t)1 << 20;  // n_wide_max: a workgroup per list entry is launched without a host wait
static_assert((SEARCH_WIDE_MAX_GATHER & (SEARCH_WIDE_MAX_GATHER - 1)) == 0 && SEARCH_WIDE_CHUNK == SEARCH_WIDE_THREADS &&
                  4 * SEARCH_WIDE_MAX_GATHER + 4 * (SEARCH_MAX_MEMBERS + 1) + 16 * SEARCH_WIDE_CHUNK + 256 <= 160 * 1024,
              "search_seeds_wide.hip: one workgroup's LDS is a CU's 160 KB at most; a round of entries fits an empty chunk");
// a window of the count pass that search_window_wide_kernel can take (include/sedef_hip.h: SDF_SEARCH_WIDE_DONE)
__host__ __device__ inline bool search_wide_eligible(const sdf_search_window &W) {
  return (W.flags & (SDF_SEARCH_WIDE | SDF_SEARCH_FOUND_WIDE)) && !(W.flags & SDF_SEARCH_NOLIMIT) && W.n_members <= SEARCH_MAX_MEMBERS &&
         W.n_gathered <= SEARCH_WIDE_MAX_GATHER;
}
__global__ void search_wide_list_kernel(const sdf_search_window *, int, uint32_t, uint32_t *, unsigned long long *, unsigned long long *);
template <bool EMIT, bool FOUND>
__global__ void search_window_wide_kernel(const sdf_minimizer *, int, long long, const sdf_minimizer *, const SearchLook *, int, int,
                                          const int32_t *, int, sdf_search_window *, uint32_t *, const uint64_t *, sdf_search_interval *,
                                          uint64_t, FoundIndex, const uint32_t *, const unsigned long long *, uint32_t);
// search_roll.hip
constexpr int ROLL_MAX_SPAN = SDF_ROLL_MAX_SPAN, ROLL_MAX_KEYS = SEARCH_MAX_MEMBERS + ROLL_MAX_SPAN;  // a wavefront's LDS: 32-bit keys, 16-bit slots
static_assert(ROLL_MAX_KEYS < 65535 && sizeof(sdf_search_roll_rec) == 24, "search_roll.hip: slots are 16 bits wide; include/sedef_hip.h");
// WALK false (profiles/search_roll.py): the set-up alone, and a record that is not the interval's
template <bool WALK>
__global__ void search_roll_kernel(const sdf_minimizer *, int, const sdf_search_window *, const uint64_t *, const sdf_search_interval *,
                                   const sdf_minimizer *, int, long long, int, const int32_t *, int, sdf_search_roll_rec *);
// search_filter.hip
constexpr int FILTER_WAVE_MAX_LEN = SDF_FILTER_WAVE_MAX_LEN, FILTER_LONG_WAVES = 4, FILTER_GRAMS = 1024;
static_assert(FILTER_WAVE_MAX_LEN < 65536, "search_filter.hip: the wavefront class counts in 16 bits");
static_assert(sizeof(sdf_filter_task) == 32 && sizeof(sdf_filter_rec) == 20 && sizeof(sdf_filter_params) == 32, "include/sedef_hip.h");
// minqg of include/sedef_hip.h, the one form the kernel and sdf_search_filter_host share: no contraction into a fused
// multiply-add on either side
__host__ __device__ inline int32_t filter_minqg(const int32_t l, const sdf_filter_params &P) {
#pragma clang fp contract(off)
  const double v = l * (1 - (P.max_error - P.max_edit_error) - 5 * P.max_edit_error) - (P.gap_frequency * l + 1) * 4;
  return v >= 2147483647.0 ? 2147483647 : v <= -2147483648.0 ? (int32_t)-2147483647 - 1 : v != v ? 0 : (int32_t)v;
}
// a task nobody reads (device forms): a range that does not lie in the pool, an unknown flag, reserved != 0
__host__ __device__ inline bool filter_task_bad(const sdf_filter_task &T, const long long pool_bytes) {
  const auto outside = [&](long long off, long long len) { return off < 0 || len < 0 || off > pool_bytes || len > pool_bytes - off; };
  return (T.flags & ~(uint32_t)(SDF_FILTER_Q_RC | SDF_FILTER_R_RC | SDF_FILTER_SKIP)) || T.reserved != 0 || outside(T.q_off, T.q_len) ||
         outside(T.r_off, T.r_len);
}
// the verdict of a pair's counts
__host__ __device__ inline sdf_filter_rec filter_verdict(int32_t q_up, int32_t r_up, int32_t dist, int32_t l, const sdf_filter_params &P) {
  sdf_filter_rec R{q_up, r_up, dist, filter_minqg(l, P), 0u};
  if (q_up < P.min_uppercase || r_up < P.min_uppercase) R.flags = SDF_FILTER_UPPER_FAIL;
  else if (dist < R.minqg) R.flags = SDF_FILTER_QGRAM_FAIL;
  if (R.minqg < 10) R.flags |= SDF_FILTER_SHORT;
  return R;
}
// WAVES wavefronts per task: 1 (16-bit counts, every task up to FILTER_WAVE_MAX_LEN) or FILTER_LONG_WAVES (32-bit counts, the
// others); a workgroup whose task is of the other class leaves at once.  REV as for the stats kernels.  MINSUM false
// (profiles/search_filter.py): the histogram pass alone, and a record that is not the pair's.
// A launch takes at most FILTER_LAUNCH_TASKS tasks: a grid of more than 2^32 - 1 lanes is refused.
constexpr size_t FILTER_LAUNCH_TASKS = (size_t)1 << 22;
template <int WAVES, bool REV, bool MINSUM>
__global__ void search_filter_kernel(const sdf_filter_task *, int, const char *, long long, sdf_filter_params, sdf_filter_rec *);
// the scalars of sdf_search_filter_tasks_*, and the task of one rolled interval of window W whose query minimizer lies at q_loc
// (include/sedef_hip.h states the rules); the one form the kernel and the host form share
struct FilterTaskArgs {
  long long len_q, len_r, q_off, r_off;
  int init_len, q_rc, r_rc, allow_extend;
};
__host__ __device__ inline sdf_filter_task filter_task_of(const FilterTaskArgs &A, const long long q_loc, const sdf_search_window &W,
                                                          const sdf_search_interval &T, const sdf_search_roll_rec &R) {
  const sdf_filter_task skip{0, 0, 0, 0, SDF_FILTER_SKIP, 0};
  if (R.jaccard < 0 || (R.flags & SDF_ROLL_BADWINDOW) || ((R.flags & SDF_ROLL_WIDE) && R.ref_end == 0) ||
      (W.flags & (SDF_SEARCH_SHORT | SDF_SEARCH_NOLIMIT)))
    return skip;
  const long long qa = q_loc, qb = q_loc + A.init_len;
  long long ra = R.ref_start, rb = R.ref_end;
  if (A.allow_extend) {  // where the walk ended
    const long long start = T.start, end = T.end, e0 = start + A.init_len < A.len_r ? start + A.init_len : A.len_r;
    long long steps = end - start < A.len_r - e0 ? end - start : A.len_r - e0;
    steps = steps < 0 ? 0 : steps;
    ra = start + steps, rb = e0 + steps;
  }
  if (qa < 0 || qb > A.len_q || ra < 0 || rb < ra || rb > A.len_r) return skip;
  sdf_filter_task O;
  O.q_off = A.q_rc ? A.q_off + A.len_q - qb : A.q_off + qa;
  O.r_off = A.r_rc ? A.r_off + A.len_r - rb : A.r_off + ra;
  O.q_len = (int32_t)(qb - qa), O.r_len = (int32_t)(rb - ra);
  O.flags = (A.q_rc ? SDF_FILTER_Q_RC : 0u) | (A.r_rc ? SDF_FILTER_R_RC : 0u), O.reserved = 0;
  return O;
}
__global__ void search_filter_tasks_kernel(const sdf_minimizer *, int, const sdf_search_window *, const uint64_t *,
                                           const sdf_search_interval *, const sdf_search_roll_rec *, int, FilterTaskArgs,
                                           sdf_filter_task *);
// search_extend.hip
// a wavefront's LDS: the members and the roll span, and EXT_GROW records on either end of either side; seven bytes a key
constexpr int EXT_GROW = SDF_EXTEND_MAX_GROW, EXT_MAX_Q = SEARCH_MAX_MEMBERS + 2 * EXT_GROW, EXT_MAX_R = ROLL_MAX_SPAN + 2 * EXT_GROW,
              EXT_MAX_KEYS = EXT_MAX_Q + EXT_MAX_R;
static_assert(EXT_MAX_KEYS < 65535 && 7 * EXT_MAX_KEYS <= 80 * 1024, "search_extend.hip: slots are 16 bits wide, two wavefronts share a CU's 160 KB");
static_assert(sizeof(sdf_search_hit) == 40 && sizeof(sdf_extend_params) == 32, "include/sedef_hip.h");
// Which intervals run, which do not fit a wavefront's replay, and the three stop tests of a round (0: go on; 1: aln_len >
// max_match, 2: the length ratio, 3: the overlap of one genome) as include/sedef_hip.h states them: the one form the kernel and
// the host form share.  lo: the first record of r with loc >= the interval's start.
__host__ __device__ inline bool extend_skips(const sdf_search_roll_rec &R, const sdf_filter_rec *F, const long long lo, const long long nr) {
  if (R.jaccard < 0 || (R.flags & SDF_ROLL_BADWINDOW) || ((R.flags & SDF_ROLL_WIDE) && R.ref_end == 0)) return true;
  if (F && (F->flags & (SDF_FILTER_UPPER_FAIL | SDF_FILTER_QGRAM_FAIL | SDF_FILTER_SKIPPED))) return true;
  return !(lo <= R.winnow_start && R.winnow_start <= R.winnow_end && R.winnow_end <= nr);
}
__host__ __device__ inline bool extend_replay_wide(const sdf_search_roll_rec &R, const int n_members, const long long lo) {
  return (R.flags & SDF_ROLL_WIDE) || n_members > SEARCH_MAX_MEMBERS || R.winnow_end - lo > ROLL_MAX_SPAN;
}
__host__ __device__ inline int extend_stops(const sdf_extend_params &P, const int qs, const int qe, const int rs, const int re) {
#pragma clang fp contract(off)
  const double gap = P.max_error - P.max_edit_error;
  int max_match = P.max_sd_size;
  if (P.same_genome) {
    const int apart = qs > rs ? qs - rs : rs - qs;
    const double v = (1.0 / gap + .5) * apart;
    const int m = v >= 2147483647.0 ? 2147483647 : v <= -2147483648.0 ? (int)-2147483647 - 1 : v != v ? 0 : (int)v;
    max_match = m < max_match ? m : max_match;
  }
  const int a = qe - qs, b = re - rs, aln_len = a > b ? a : b, seq_len = a > b ? b : a;
  if (aln_len > max_match) return 1;
  if (100.0 * (double)seq_len / (double)aln_len < 100 * (1 - 2 * gap)) return 2;
  if (P.same_genome) {
    const int overlap = qe - rs;
    if (overlap > 0 && 100.0 * (double)overlap / (double)b > 100 * P.max_error) return 3;
  }
  return 0;
}
__global__ void search_extend_kernel(const sdf_minimizer *, int, const sdf_search_window *, const uint64_t *, const sdf_search_interval *,
                                     const sdf_search_roll_rec *, const sdf_filter_rec *, const sdf_minimizer *, int, long long, long long, int,
                                     const int32_t *, int, sdf_extend_params, sdf_search_hit *);
// the filter task of a hit (include/sedef_hip.h: sdf_search_hit_tasks_*); of A, init_len and allow_extend are not read
__host__ __device__ inline sdf_filter_task hit_task_of(const FilterTaskArgs &A, const sdf_search_hit &H) {
  const sdf_filter_task skip{0, 0, 0, 0, SDF_FILTER_SKIP, 0};
  if ((H.flags & (SDF_EXTEND_SKIPPED | SDF_EXTEND_NOLIMIT)) || ((H.flags & SDF_EXTEND_WIDE) && H.query_end == 0)) return skip;
  const long long qa = H.query_start, qb = H.query_end, ra = H.ref_start, rb = H.ref_end;
  if (qa < 0 || qb < qa || qb > A.len_q || ra < 0 || rb < ra || rb > A.len_r) return skip;
  sdf_filter_task O;
  O.q_off = A.q_rc ? A.q_off + A.len_q - qb : A.q_off + qa;
  O.r_off = A.r_rc ? A.r_off + A.len_r - rb : A.r_off + ra;
  O.q_len = (int32_t)(qb - qa), O.r_len = (int32_t)(rb - ra);
  O.flags = (A.q_rc ? SDF_FILTER_Q_RC : 0u) | (A.r_rc ? SDF_FILTER_R_RC : 0u), O.reserved = 0;
  return O;
}
__global__ void search_hit_tasks_kernel(const sdf_search_hit *, int, const uint64_t *, FilterTaskArgs, sdf_filter_task *);
// search_extend_long.hip
// a wavefront's LDS: bits[] alone, one byte per key of the largest universe; the keys' sort and the slots lie in HBM
constexpr int EXT_LONG_GROW = SDF_EXTEND_LONG_MAX_GROW, EXT_LONG_MAX_KEYS = SEARCH_MAX_MEMBERS + ROLL_MAX_SPAN + 4 * EXT_LONG_GROW;
static_assert(EXT_LONG_MAX_KEYS <= 80 * 1024, "search_extend_long.hip: two wavefronts share a CU's 160 KB");
constexpr uint32_t kLongNoSlot = 0xFFFFFFFFu, kLongPayloadNoSlot = 0x80000000u;  // a status-2 reference record: in slots[], in the sort's payload
constexpr int kLongPadBit = 32, kLongSlotShift = 33;                              // a sort key: slot << 33 | pad << 32 | roll_key
struct ExtLongCand {  // a taken candidate: its interval, its window, the first record of r with loc >= the interval's start
  uint32_t t;
  int32_t i, lo;
};
struct ExtLongArgs {  // what the launches of sdf_search_extend_long_device share
  const sdf_minimizer *q, *r;
  const sdf_search_window *windows;
  const uint64_t *first;
  const sdf_search_interval *intervals;
  const sdf_search_roll_rec *rolls;
  const sdf_filter_rec *filter;
  int nq, nr, n_limit, grow, stride;  // grow: long_grow; stride: U, the universe entries a batch slot owns
};
__global__ void search_extend_long_flag_kernel(ExtLongArgs, const sdf_search_hit *, int, uint32_t *);
__global__ void search_extend_long_list_kernel(ExtLongArgs, const sdf_search_hit *, const uint32_t *, const uint32_t *, int, uint32_t, ExtLongCand *, uint32_t *,
                                               unsigned long long *);
__global__ void search_extend_long_keys_kernel(ExtLongArgs, const ExtLongCand *, const uint32_t *, uint32_t, unsigned long long *, uint32_t *);
__global__ void search_extend_long_heads_kernel(const unsigned long long *, int, int, uint32_t *);
__global__ void search_extend_long_slots_kernel(const unsigned long long *, const uint32_t *, const uint32_t *, int, int, uint32_t *, uint32_t *);
__global__ void search_extend_long_kernel(ExtLongArgs, const ExtLongCand *, const uint32_t *, uint32_t, const uint32_t *, const uint32_t *,
                                          long long, long long, int, const int32_t *, sdf_extend_params, sdf_search_hit *, unsigned long long *);
// search_accept.hip
// a wavefront's LDS: the kept records of its window, their intervals' indices and a byte each
constexpr int ACCEPT_MAX_KEPT = SDF_ACCEPT_MAX_KEPT;
constexpr int ACCEPT_KEPT_BYTES = (int)(sizeof(sdf_search_found) + sizeof(uint32_t) + sizeof(uint8_t));  // record, interval index, dropped
static_assert(ACCEPT_MAX_KEPT >= 64 && ACCEPT_MAX_KEPT % 64 == 0 && ACCEPT_MAX_KEPT * ACCEPT_KEPT_BYTES <= 160 * 1024 / 15,
              "search_accept.hip: fifteen wavefronts share a CU's 160 KB (include/sedef_hip.h)");
static_assert(sizeof(sdf_search_pair_hit) == 24 && sizeof(sdf_search_accept_status) == 64, "include/sedef_hip.h");
struct AcceptRound {  // sdf_search_accept_round as the kernels take it
  const sdf_minimizer *q;
  const uint32_t *act;
  const sdf_search_window *windows;
  const uint64_t *first;
  const sdf_search_roll_rec *rolls;
  const uint32_t *overlap;
  const sdf_filter_rec *filter;
  const sdf_search_hit *hits;
  const sdf_filter_rec *hit_filter;
  long long n_max;
  int nq, na, init_len, min_read_size, window_base;
};
struct AcceptWin {  // what the first launch leaves per round window (32 bytes)
  int32_t n_kept, n_out, reach, incomplete;  // reach: the largest q_end of a kept record, 0: none
  int32_t attempted, jaccard_failed, interval_failed, qs;
};
struct AcceptOff {  // where an accepted window's records go, counted from nf and n_out
  uint32_t found, out;
};
constexpr uint32_t kAcceptDropped = 0x80000000u;  // in a kept entry: parse_hits dropped the hit
// An interval's class in the acceptance step (include/sedef_hip.h): 0 jaccard failed, 1 overlapped by the found list as it stood,
// 2 goes on to the replay of is_overlap but cannot be kept, 3 a candidate; and whether the device left its record for the host.
// The one form the kernel and the host form share.
__host__ __device__ inline int accept_class(const sdf_search_roll_rec &R, const uint32_t verdict, const sdf_filter_rec &F,
                                            const sdf_search_hit &H, const sdf_filter_rec &HF) {
  constexpr uint32_t fail = SDF_FILTER_UPPER_FAIL | SDF_FILTER_QGRAM_FAIL | SDF_FILTER_SKIPPED;
  if (R.jaccard < 0) return 0;
  if (verdict) return 1;
  return (F.flags & fail) || (H.flags & (SDF_EXTEND_SKIPPED | SDF_EXTEND_NOLIMIT)) || (HF.flags & fail) ? 2 : 3;
}
__host__ __device__ inline bool accept_unfinished(const sdf_search_roll_rec &R, const sdf_search_hit &H) {
  return ((R.flags & SDF_ROLL_WIDE) && R.ref_end == 0) || (R.flags & SDF_ROLL_BADWINDOW) || ((H.flags & SDF_EXTEND_WIDE) && H.query_end == 0);
}
// parse_hits: p makes h drop
__host__ __device__ inline bool accept_contains(const sdf_search_found &p, const sdf_search_found &h) {
  return h.r_start >= p.r_start && h.r_end <= p.r_end && h.q_start >= p.q_start && h.q_end <= p.q_end;
}
__global__ void search_accept_window_kernel(AcceptRound, AcceptWin *, uint32_t *);
__global__ void search_accept_frontier_kernel(const AcceptWin *, int, unsigned long long, unsigned long long, unsigned long long,
                                              unsigned long long, AcceptOff *, sdf_search_accept_status *, uint32_t *);
__global__ void search_accept_tail_kernel(uint64_t *, int, int);
__global__ void search_accept_append_kernel(AcceptRound, const AcceptWin *, const uint32_t *, const AcceptOff *, const uint32_t *,
                                            sdf_search_found *, unsigned long long, unsigned long long, sdf_search_pair_hit *,
                                            unsigned long long, unsigned long long);
// pair_recall.hip (include/sedef_hip.h: sdf_pair_recall): the rule, once, for the host form and the kernels
constexpr int kRecallCap = SDF_RECALL_CAP;
constexpr unsigned long long kRecallNoKey = ~0ull;  // the sort key of an end that can meet nothing: behind every key of an id
struct RecallEnd {
  int32_t chr, start, end;
  uint32_t strand;
};
__host__ __device__ inline RecallEnd recall_end(const sdf_pair_rec &r, const int e) {
  return e ? RecallEnd{r.chr2, r.start2, r.end2, (r.flags >> 1) & 1u} : RecallEnd{r.chr1, r.start1, r.end1, r.flags & 1u};
}
__host__ __device__ inline bool recall_rec_bad(const sdf_pair_rec &r) {
  return r.chr1 < 0 || r.chr2 < 0 || r.start1 < 0 || r.start2 < 0 || r.start1 > r.end1 || r.start2 > r.end2 || r.reserved != 0 || (r.flags & ~3u);
}
// (ends of checked records: 0 <= start <= end, so neither difference leaves an int)
__host__ __device__ inline bool recall_meets(const RecallEnd &a, const RecallEnd &b, const bool ignore_strand) {
  const int32_t lo = a.start > b.start ? a.start : b.start, hi = a.end < b.end ? a.end : b.end;
  return a.chr == b.chr && hi - lo >= 1 && (ignore_strand || a.strand == b.strand);
}
// end f of a hitting record clipped to the gold end g it meets, counted from g's first base: start << 32 | end, 0 <= start < end
__host__ __device__ inline unsigned long long recall_clip(const RecallEnd &g, const RecallEnd &f) {
  const int32_t lo = (f.start > g.start ? f.start : g.start) - g.start, hi = (f.end < g.end ? f.end : g.end) - g.start;
  return (unsigned long long)(uint32_t)lo << 32 | (uint32_t)hi;
}
__host__ __device__ inline unsigned long long recall_key(const int32_t chr, const long long start) {
  return (unsigned long long)(uint32_t)chr << 32 | (uint32_t)(start < 0 ? 0 : start);
}
// The candidates of a gold end [start, end) among ends sorted by recall_key, none longer than max_len: the keys in
// [recall_key(chr, start - max_len + 1), recall_key(chr, end)) -- an end that starts at or below start - max_len stops at or
// below start, one that starts at `end` or behind it starts behind the gold end.
// What entry (record F, end p) says about gold record G, whose end 1 the entry is a candidate of: *hit -- F's end p meets G.1 and
// its other end G.2 (p == 0: directly, p == 1: crosswise) --, *counts -- this entry is the one of F's that n_hits counts: the
// direct one, or the crosswise one of a record without a direct hit --, and the two clipped intervals.
__host__ __device__ inline void recall_entry(const sdf_pair_rec &G, const sdf_pair_rec &F, const int p, const bool ignore_strand, bool *hit,
                                             bool *counts, unsigned long long *iv1, unsigned long long *iv2) {
  const RecallEnd g1 = recall_end(G, 0), g2 = recall_end(G, 1), a = recall_end(F, p), b = recall_end(F, 1 - p);
  *hit = recall_meets(g1, a, ignore_strand) && recall_meets(g2, b, ignore_strand);
  *counts = *hit && (p == 0 || !(recall_meets(g1, b, ignore_strand) && recall_meets(g2, a, ignore_strand)));
  *iv1 = *hit ? recall_clip(g1, a) : 0ull;
  *iv2 = *hit ? recall_clip(g2, b) : 0ull;
}
__global__ void recall_entries_kernel(const sdf_pair_rec *, int, unsigned long long *, uint32_t *, int32_t *, unsigned long long *);
__global__ void recall_kernel(const sdf_pair_rec *, const sdf_pair_rec *, const unsigned long long *, const uint32_t *, int, const int32_t *,
                              uint32_t, sdf_pair_recall_rec *, unsigned long long *);
// line_order.hip (include/sedef_hip.h: sdf_line_order): what the host form and the kernels ask of a line, once
constexpr int kLineRun = SDF_LINE_RUN;
__host__ __device__ inline bool line_rec_bad(const sdf_line_rec &r, const unsigned long long pool_bytes) {
  return (r.off & 15u) != 0 || r.reserved != 0 || r.off > pool_bytes || r.len > pool_bytes - r.off;
}
__host__ __device__ inline bool line_keys_equal(const sdf_line_rec &a, const sdf_line_rec &b) {
  bool same = true;
  for (int k = 0; k < 8; k++) same &= a.key[k] == b.key[k];
  return same;
}
__global__ void line_keys_kernel(const sdf_line_rec *, const uint32_t *, uint32_t *, unsigned long long *, int, int, unsigned long long,
                                 uint32_t *);
__global__ void line_heads_kernel(const sdf_line_rec *, const uint32_t *, int, uint8_t *, uint32_t *, uint32_t *, uint32_t *, uint32_t *);
__global__ void line_tie_kernel(const uint8_t *, unsigned long long, const sdf_line_rec *, int, const uint8_t *, const uint32_t *,
                                const uint32_t *, uint32_t *, uint32_t *, uint32_t *);

}  // namespace sdf
