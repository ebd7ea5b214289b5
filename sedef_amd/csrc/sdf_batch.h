// What the three host pieces of a batch call share: the planner's records (sdf_plan.hip), the progress of a call on the
// device (sdf_launch.hip) and the functions the batch entry points (sdf_api.hip) call in them.
#pragma once
#include <utility>

#include "sdf_ctx.h"

namespace sdf {

inline const sdf_config *default_config() {  // (a PlanEnv nobody gave a context's settings: the library's defaults)
  static const sdf_config c = [] {
    sdf_config d;
    sdf_config_default(&d);
    return d;
  }();
  return &c;
}

// What the planner reads: the context's settings (cfg, sdf_config.hip) and what is derived from them, the scoring and
// the request per call (sdf_api.hip: plan_env fills it).
struct PlanEnv {
  const sdf_config *cfg = default_config();
  const sdf_task *tasks = nullptr;
  size_t n = 0;
  uint32_t want = 0;
  bool degenerate = false;  // scoring for which the reference returns before any work (:81)
  int gapo = 0;
  int max_dyn_lds = 64 * 1024;
  bool force_general = false;  // SDF_FORCE_GENERAL, or a scoring the window kernels do not take
  bool strip_ok = false;       // strip kernels (extz2_strip.hip) allowed: the scoring is tame
  // lane kernel (extz2_lane.hip): small full-band tasks leave the host's planning altogether when the batch holds at least
  // SDF_LANE_MIN of them (fewer do not fill the device: a lane walks its matrix alone, ~100 cycles per cell)
  bool lane_ok = false;          // the scoring is tame and only CIGAR / score / mte are wanted
  LaneRec *lane_recs = nullptr;  // pinned, one per task of the batch: filled by the scan (none: no lane kernel)
  bool want_cigar() const { return (want & SDF_WANT_CIGAR) != 0; }
};

// Launch class: the kernel instantiation a launch runs (sdf_launch.hip: launch_dp).
struct LaunchClass {
  enum class Family { Wave, Pair, PairTrack, PairMixed, Stripe, BStripe, Strip, Chain, General, GeneralPlain, GeneralHbm, GeneralPlainHbm };
  Family fam;
  int nreg = 0;         // window registers (wave, pair kernels), stripe width (stripe kernels), columns per lane (chains)
  bool stream = false;  // wave / pair kernel: the streamed-window instantiation (sequences longer than the LDS windows)
  int block = 0;        // general kernels: threads per workgroup
  bool operator==(const LaunchClass &o) const { return fam == o.fam && nreg == o.nreg && stream == o.stream && block == o.block; }
  bool operator!=(const LaunchClass &o) const { return !(*this == o); }
  // one launch-order entry per stripe, (stripe << 24) | task (chains: per block of a pair of tasks)
  bool per_stripe() const { return fam == Family::Stripe || fam == Family::BStripe || fam == Family::Chain; }
  // an entry holds two tasks: a task and its partner (itself, when it has none), one wavefront
  bool two_per_entry() const { return fam == Family::Pair || fam == Family::PairTrack || fam == Family::PairMixed || fam == Family::Strip; }
  bool hbm_state() const { return fam == Family::GeneralHbm || fam == Family::GeneralPlainHbm; }  // lds = slab bytes per workgroup
  bool mixed() const { return fam == Family::PairMixed; }  // long and short banded tasks in one launch
  // rough cells per unit of time of one workgroup (the duration estimate of a class)
  double rate() const {
    switch (fam) {
      case Family::Wave: return 0.13;
      case Family::Pair: case Family::PairTrack: case Family::PairMixed: return 0.25;
      case Family::Stripe: return 1.0;
      case Family::BStripe: return 0.3;
      case Family::Strip: return 0.5;
      case Family::Chain: return 2.0;
      case Family::General: return block == 64 ? 0.03 : block == 256 ? 0.1 : 0.6;
      case Family::GeneralPlain: return block == 256 ? 0.3 : 0.85;
      case Family::GeneralHbm: return 0.08;
      case Family::GeneralPlainHbm: return 0.3;
    }
    return 0.13;
  }
  // The number SDF_DEBUG_CLASSES prints and sdf_debug_plan reports: 1..8 wave kernel with NREG (+10 streamed windows), 100 +
  // NREG pair kernel (+10 streamed; 120 + NREG TRACK, 130 + NREG MIXED flavour), 300 / 400 + NREG stripe / banded stripe
  // kernel, 500 strip kernel, 600 + columns per lane chained strips, 64 / 256 / 1024 general kernel with that many threads
  // (+2000 PLAIN flavour), 1000 / 1001 / 2001 general kernel with its state in HBM (256 / 1024 threads, PLAIN).
  int code() const {
    switch (fam) {
      case Family::Wave: return nreg + (stream ? 10 : 0);
      case Family::Pair: return 100 + nreg + (stream ? 10 : 0);
      case Family::PairTrack: return 120 + nreg;
      case Family::PairMixed: return 130 + nreg;
      case Family::Stripe: return 300 + nreg;
      case Family::BStripe: return 400 + nreg;
      case Family::Strip: return 500;
      case Family::Chain: return 600 + nreg;
      case Family::General: return block;
      case Family::GeneralPlain: return 2000 + block;
      case Family::GeneralHbm: return block == 1024 ? 1001 : 1000;
      case Family::GeneralPlainHbm: return 2001;
    }
    return -1;
  }
};

struct Launch {
  LaunchClass lc;
  size_t lds;  // dynamic LDS bytes of the launch (HBM-state classes: slab bytes per workgroup)
  size_t off, cnt;  // entries of the chunk's launch order
  double est;       // duration estimate: the launch's longest task
  int rmax = 0;     // stripe kernel: anti-diagonals (qlen + tlen) of the launch's longest task
};

struct ChunkPlan {
  size_t s = 0, e = 0;   // ordinary chunk: task range [s, e) of the caller's array, minus the heavy tasks in it;
  bool heavy = false;    // heavy chunk: range [s, e) of BatchCut::heavy_idx
  size_t pb = 0;         // first PlanTask of the chunk
  size_t ob = 0;         // first launch-order entry (room for `order_cap`: a task paired with itself is listed twice,
                         // a stripe task once per stripe)
  size_t order_cap = 12288;  // (up to five stripe launches -- one width of the full-band kernel, three of the banded one -- of up
                             // to 8 x 254 idle entries each)
  int64_t stage0 = 0;    // first CIGAR staging word
  size_t ntask = 0;      // tasks the chunk will plan (known after cut_batch)
  int64_t stage_words = 0;  // CIGAR staging words of those tasks
  // filled by plan_chunk
  size_t cnt = 0, nord = 0;
  std::vector<Launch> launches;
  unsigned layouts = 0;  // direction-flag layouts present: bit 0 byte rows, 1 wave blocks, 2 pair blocks, 3 stripes
  long long paired = 0;
  size_t dir_bytes = 0;
  const char *err = nullptr;
};

#define SDF_CUT_BLOCK 4096

struct BatchCut {
  std::vector<ChunkPlan> chunks;  // heavy chunks first
  std::vector<uint8_t> heavy;     // per task, when split_heavy
  std::vector<uint32_t> heavy_idx;  // the heavy tasks, ascending
  // scratch of cut_batch, kept by the context between calls (fresh vectors of this size cost a millisecond of page faults)
  std::vector<uint32_t> bound;      // per task: upper bound of its direction flags, in units of 256 bytes
  std::vector<uint32_t> cap;        // per task: CIGAR staging words | 0x80000000 when the task runs at all
  std::vector<uint32_t> hparts[16];  // heavy task indices, per scan thread
  std::vector<sdf_task> htasks[16];  // ... and their records: plan_chunk reads the heavy tasks from a compact copy (they lie
                                     // scattered over the caller's array -- a cache miss each, on the thread in front of the
                                     // call's first launch)
  std::vector<sdf_task> heavy_tasks;  // the records of heavy_idx, in its order
  struct Block {  // sums over SDF_CUT_BLOCK consecutive tasks: all runnable ones / the heavy ones / the lane tasks among them
    uint64_t bd = 0, hbd = 0;  // direction-flag bounds, bytes
    uint32_t nt = 0, hnt = 0, sw = 0, hsw = 0, oc = 0, hoc = 0;  // tasks, CIGAR staging words, launch-order entries
    uint32_t lnt = 0, lsw = 0;  // lane tasks (not in the sums above) and their staging words
    uint64_t ldir = 0;          // direction-flag bytes of the lane tasks in the lane kernel's own layout
    uint32_t lcls[4] = {0, 0, 0, 0};  // lane tasks per launch class (query length)
  };
  std::vector<Block> blocks;
  void reset() {
    chunks.clear();
    heavy_idx.clear();
    split_heavy = pipelined = false;
    nch = max_regions = nreg_ws = 1;
    n_heavy = 0;
    region_need = 16;
    heavy_need = 0;
    stage_total = 0;
    ntask_total = 0;
    order_total = 0;
    use_lane = false;
    n_early = 0;
    stage_upper = 0;
    order_upper = 0;
    n_lane = 0;
    lane_stage_words = 0;
    lane_dir_bytes = 0;
    for (auto &c : lane_cls) c = 0;
  }
  // lane kernel: tasks the scan found eligible (lane[k] != 0), taken out of the chunks when there are enough of them
  std::vector<uint8_t> lane;
  bool use_lane = false;
  size_t n_lane = 0, lane_cls[4] = {0, 0, 0, 0};
  int64_t lane_stage_words = 0;
  size_t lane_dir_bytes = 0;
  bool split_heavy = false, pipelined = false;
  size_t nch = 1, max_regions = 1, n_heavy = 0;
  size_t region_need = 16, heavy_need = 0, nreg_ws = 1;
  int64_t stage_total = 0;
  size_t ntask_total = 0;
  size_t order_total = 0;
  // early start (cut_batch's `early` callback): the heavy chunks are cut after a first pass over the BIG tasks only and
  // handed to the caller -- which plans and launches them -- while the pass over the rest of the batch runs
  size_t n_early = 0;         // chunks of `chunks` (its first ones, all heavy) that the callback has launched
  int64_t stage_upper = 0;    // upper bound of stage_total + the lane tasks' words, known after the first pass
  size_t order_upper = 0;     // upper bound of order_total
};

namespace plan_detail {

// stripe width of the banded stripe kernel: the narrowest with at most 254 stripes (0: target too long)
inline int bstripe_nreg(int tlen, const int forced) {  // forced: sdf_config.bstripe_nreg (tests: wider stripes than the target needs)
  const int t16 = (tlen + 15) / 16 * 16;
  if ((forced == 2 || forced == 4) && t16 <= 254 * 128 * forced) return forced;
  return t16 <= 254 * 128 ? 1 : t16 <= 254 * 256 ? 2 : t16 <= 254 * 512 ? 4 : 0;
}

inline bool task_runs(const sdf_task &t, bool degenerate) { return t.qlen > 0 && t.tlen > 0 && !degenerate; }

struct Cls {
  LaunchClass lc;
  size_t lds;       // class key
  size_t need_max;  // largest real requirement in the class: what the launch asks for
  std::vector<int32_t> idx;
  double est = 0;
};

}  // namespace plan_detail

// Per-thread scratch of plan_chunk (kept between chunks: no allocation in the steady state).
struct PlanScratch {
  std::vector<int32_t> win_need, partner;
  std::vector<std::pair<int32_t, int32_t>> table;
  std::vector<plan_detail::Cls> cls;
  std::vector<char> tracked, mixedf;
  std::vector<int32_t> bs_alt;       // tasks given to the banded stripe kernel that a mixed pair could take: index, wave nreg, window need
  std::vector<uint64_t> mix_keys;
  std::vector<int32_t> stripe_lane, stripe_fill;
  std::vector<uint64_t> strip_keys, strip_keys_tmp;
};

// ---- sdf_plan.hip ----
// Returns SDF_OK or an error code with *err set.  `early`: see the definition.
int cut_batch(const PlanEnv &env, bool pipeline_enabled, size_t ws_budget, BatchCut &cut, const char **err,
              WorkerPool *pool = nullptr, const std::function<int()> *early = nullptr);
// Plans one chunk into plan[c.pb ...] and order[c.ob ...].
void plan_chunk(const PlanEnv &env, const BatchCut &cut, ChunkPlan &c, PlanTask *plan, int32_t *order, PlanScratch &sx);

// ---- sdf_launch.hip ----
struct ChunkEv {
  hipEvent_t dp0 = nullptr, dpe[16] = {}, tb0 = nullptr, tb1 = nullptr;  // plan uploaded; end of the DP launches per
                                                                         // stream; traceback (begin, end)
};

// Progress of one batch call on the device.
struct BatchRun {
  sdf_ctx *ctx = nullptr;
  hipStream_t st = nullptr;  // the caller's stream
  ScoreK sk;
  const uint32_t *d_pool = nullptr;
  sdf_result *d_out = nullptr;
  PlanTask *plan = nullptr, *d_plan = nullptr;  // pinned host copy / device copy
  int32_t *order = nullptr, *d_order = nullptr;
  uint8_t *d_dir = nullptr;
  uint8_t *heavy_dir = nullptr;  // the heavy chunks' slice (the workspace as it was when they were launched)
  size_t claim_sets = 0;         // stripe launches of the call so far (each has eight entry counters in ctx->claim_buf)
  bool more_chunks = false;      // early start: chunks of ordinary tasks will follow those in cut->chunks
  uint32_t *d_stage = nullptr;
  const BatchCut *cut = nullptr;
  bool want_cigar = false, have_heavy = false;
  std::vector<ChunkEv> cev;
  std::vector<size_t> normal_ids;  // chunk indices of the ordinary chunks launched so far
  double qload[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // estimated DP work queued on each stream during this call
  size_t evc = 0;
  hipEvent_t ev_begin = nullptr;
  bool any_stripe = false;  // a stripe kernel was launched: its give-up list is looked at before the batch closes
  const sdf_scoring *scoring = nullptr;  // what the caller passed (a re-run of abandoned tasks passes them on)
  const sdf_task *tasks = nullptr;
  uint32_t want = 0;
  hipEvent_t ev_lane = nullptr;  // the lane tasks' DP and traceback have finished
  hipEvent_t ev_lane0 = nullptr;  // ... are about to start (debug timing)
  hipStream_t began[24] = {};  // internal streams already ordered behind ev_begin in this call
  size_t nbegan = 0;
};

hipEvent_t next_event(sdf_ctx *ctx, size_t &cursor);
void drain_streams(sdf_ctx *ctx, hipStream_t st);  // every stream a batch call may have work on
int launch_chunk(BatchRun &run, size_t ci);
hipError_t create_lane_stream(const sdf_ctx *ctx, hipStream_t *out);
int launch_lane(BatchRun &run, size_t n);
int finish_batch(BatchRun &run, BatchRun *head, size_t n, sdf_result *d_out, uint32_t *d_cig, size_t cigar_cap,
                 size_t *cigar_used);

}  // namespace sdf
