// Batch planning for the DP entry points (host code only; no device work happens in this file).
//
//   cut_batch()   one pass over the caller's tasks: validation, upper bounds of the direction-flag bytes, the split of
//                 "heavy" tasks from the chunk rotation, chunk boundaries, and -- so that chunks can be planned
//                 independently of each other, on several threads -- every chunk's bases into the shared arrays
//                 (PlanTask index, launch-order index, CIGAR staging word);
//   plan_chunk()  one chunk: kernel choice per task, pairing of tasks of equal geometry, the direction-flag layout
//                 inside the chunk's workspace region, launch classes and the launch order.  Pure function of the
//                 tasks and the PlanEnv: the unit tests of the planner need no GPU.
//
// Both are sequences of passes (the functions of the two unnamed namespaces below); the per-task rules they apply --
// which kernel takes what, in how many registers, with how many flag bytes -- are stated once, in sdf_plan_rules.h.
//
// Replaces the per-call set-up of ksw_extz2_sse (reference: extern/ksw2_extz2_sse.cc:57-98: early-outs, band and
// matrix geometry, allocation) for a batch of tasks.
#include "sdf_plan_rules.h"

#include <atomic>
#include <memory>
#include <thread>

namespace sdf {

// ---- cut_batch: its passes ----------------------------------------------------------------------------------------------
namespace {
using namespace plan_detail;

// What a task needs of the chunks' budgets: launch-order entries, staging words, an upper bound of its flag bytes
// whichever kernel takes it (a superset of what plan_chunk gives: the maximum of placed_dir_bytes' terms over the kinds
// the task may still take), and what "heavy" is measured by.  Pure.
struct TaskNeeds {
  uint32_t oc = 0, words = 0;
  size_t bd = 0, hvb = 0;
};

// (strip kernel: a region per PAIR of tasks with as many column blocks, sized by the one with more rows -- which
// this pass does not know.  A pair of m and M <= 1.125 m + 64 rows needs blocks x (M + 63) records of 8 bytes, a task
// without a partner blocks x (rows + 63) records of 4; every task reserves blocks x (0.54 rows + 60) x 520 bytes:
// enough for either, the chains' edge columns included -- 0.54 (1.889 M - 57) + 120 >= M + 64.  Until the end of
// round 6 the pairs were allowed M <= 1.5 m + 64 and the factor was 0.8: the far-gap round of the chr1-sized stage
// reserved 9.1 GB for flags that take 5.0, and a workspace of 8 GiB cut it in two)
// (a chain's blocks are four columns per lane wide when its chunk holds few of them -- plan_chunk decides, unless
// SDF_STRIP_COLS=8 does --: twice the blocks, a record per PAIR of steps -- the same bytes, one block of rounding
// apart, whichever plan_chunk picks)
size_t strip_reserve_bytes(const PlanEnv &env, const sdf_task &t) {
  const size_t recs = (size_t)(t.qlen * 27 / 50 + 60);
  if (chain_range(t) && env.cfg->strip_cols != 8)
    return round256((size_t)std::max(strip_blocks(t.tlen, 4), 2 * strip_blocks(t.tlen, 8)) * recs * 260 + 512);
  return round256((size_t)strip_blocks(t.tlen, 8) * recs * 520 + 512);
}

TaskNeeds task_needs(const PlanEnv &env, const sdf_task &t) {
  TaskNeeds nd;
  nd.oc = order_entries(env, t);
  const bool dir = with_dir(env, t);
  nd.words = dir ? stage_words(t) : 0u;
  const int w = resolved_w(t), need = window_need(t);
  const bool plain = simple(env, t) && !env.force_general;
  size_t bd = 0;
  if (dir) {
    // (the reference's byte per cell is the general kernel's layout: a task with nothing special asked of it, whose band
    // reaches the end and whose window a register-resident kernel holds never goes there -- choose_kind's `plain_ok`;
    // for a batch of long banded tasks the byte rows are twice the bits, and the bound is what cuts it into chunks)
    const bool bits_only = wave_nreg(need) && plain && band_whole(t) &&
                           wave_lds_bytes(t.qlen, t.tlen, wave_nreg(need)) <= (size_t)env.max_dyn_lds;
    nd.hvb = byte_rows_bytes(t.qlen, t.tlen, ncol16(t));  // (what "heavy" is measured by, whichever layout the task takes)
    // (round 6) ... nor does a wide FULL-BAND task that plan_chunk always hands to the stripe / strip / chain kernels (their
    // own bounds follow below: 0.5-0.8 bytes per cell against the byte rows' two per cell of a square matrix).  The
    // far-gap round of the chr1-sized stage -- 10,813 tasks, 9.5e9 cells -- was cut into two chunks of one 7 ms chain each
    // by that bound; one chunk: DP 14.4 -> see profiles/r06_stage_dp2.txt.
    const bool striped_always = plain && !env.cfg->no_stripe && full_band(t) && stripe_range(env, t) && stripe_lds_ok(env, t);
    if (!bits_only && !striped_always) bd = nd.hvb;
    // (the wave kernel's blocks: 1 KiB per register of 128 slots -- 1, 2, 3, 4, 6 or 8 of them; the pair kernels' 512 B per
    // register of 64 slots, up to nine, stay below)
    if (wave_nreg(need)) bd = std::max(bd, wave_dir_bytes(t.qlen, t.tlen, wave_nreg(need)));
    // (the pair kernel's TRACK flavour)
    if (track_nreg(need)) bd = std::max(bd, pair_dir_bytes(t.qlen, t.tlen, track_nreg(need)));
    // (a MIXED pair gives both tasks the register count of the wider window: a banded task of a short target may sit next
    // to one whose window is as wide as the band allows -- ((w + 1 + 15) / 16 + 1) * 16 + 32 slots, at most kMixedMaxNeed --
    // at 512 B per register and block of its OWN rows)
    if (bits_only && need <= kMixedMaxNeed && !full_band(t))
      bd = std::max(bd, pair_dir_bytes(t.qlen, t.tlen, mixed_nreg(band_window_need(w))));
  }
  if (stripe_range(env, t) && full_band(t))  // (stripe kernel, any width)
    for (int nr = 1; nr <= 4; nr *= 2) bd = std::max(bd, stripe_region_bytes(t.qlen, t.tlen, nr));
  if (banded_long(env, t)) bd = std::max(bd, bstripe_region_bytes(t.qlen, t.tlen, w, bstripe_nreg(t.tlen, (int)env.cfg->bstripe_nreg)));
  // (wider targets: a chain of wavefronts, the edge columns between the blocks behind the records -- reserved, like
  // the other stripe kernels' inter-stripe words, whatever the task wants)
  if (env.strip_ok && (strip_range(t) || chain_range(t)) && full_band(t) && (dir || chain_range(t)))
    bd = std::max(bd, strip_reserve_bytes(env, t));
  nd.bd = bd;
  return nd;
}

// (what a task needs depends on (qlen, tlen, w, SCORE_ONLY) alone, and batches repeat their geometries -- the headline
// batch has a hundred of them in 100,000 tasks: a small direct-mapped memo per scan thread)
struct Memo {
  int32_t qlen = -1, tlen = -1, w = 0, so = 0;
  TaskNeeds nd;
};
struct Part {  // one scan thread's
  size_t nh = 0, hb = 0;
  bool bad = false;
  Memo memo[256];
  int64_t words = 0;       // first pass: q + t + 2 of every task, the big tasks' launch-order entries, their number
  size_t big_oc = 0, nbig = 0;
  int64_t rows_max = 0;    // anti-diagonals of the longest task accounted for
};

// bases: what the chunks before this one (in launch order) occupy; the batch's totals once its chunks are all there
// (the early start's heavy chunks are not: the launcher reads ntask_total)
void assign_bases(BatchCut &cut, const bool whole_batch) {
  size_t pb = 0, ob = 0;
  int64_t stage = 0;
  for (ChunkPlan &c : cut.chunks) {
    c.pb = pb;
    c.ob = ob;
    c.stage0 = stage;
    pb += c.ntask;
    ob += c.order_cap;
    stage += c.stage_words;
  }
  if (!whole_batch) return;
  cut.ntask_total = pb;
  cut.order_total = ob;
  cut.stage_total = stage;
}

struct Cutter {
  const PlanEnv &env;
  BatchCut &cut;
  const size_t ws_budget;
  WorkerPool *const pool;
  const sdf_task *const tasks = env.tasks;
  const size_t n = env.n;
  const size_t nblk = (n + SDF_CUT_BLOCK - 1) / SDF_CUT_BLOCK;
  const bool lane_scan = env.lane_ok && env.lane_recs && n >= (size_t)env.cfg->lane_min;
  // A task is "heavy" when its wavefront (or workgroup) is busy for about a millisecond or more whatever else runs:
  // 500 x 500 and up at full band, i.e. from 256 KB of direction flags.
  const size_t heavy_min = env.cfg->heavy_bytes > 0 ? (size_t)env.cfg->heavy_bytes : (size_t)256 << 10;
  const size_t hv_limit = n / 4 + 1;
  const int force_nch = (int)env.cfg->cut_chunks;  // (experiments: the number of ordinary chunks a large batch is cut into)
  int nthr = 1;
  bool two_pass = false;
  bool chain_bound = false;  // (set after the scan: fewer chunks than the size of the batch alone would give)
  size_t nch_by_size = 1, first_target0 = 0;
  size_t heavy_bytes = 0, heavy_budget = 0;
  std::vector<ChunkPlan> heavy_chunks;
  Part parts[16];

  Cutter(const PlanEnv &e, BatchCut &c, size_t ws, WorkerPool *p) : env(e), cut(c), ws_budget(ws), pool(p) {}

  void decide_pipeline(bool pipeline_enabled);
  void prepare_scratch();
  void account(size_t k, Part &pt, std::vector<uint32_t> &hv, bool may_be_heavy);
  void fill_lane(size_t k);
  bool is_big(const sdf_task &t) const;
  void scan(size_t lo, size_t hi, Part &pt, std::vector<uint32_t> &hv, int mode);
  void run_pass(int mode, const std::function<void()> *meanwhile);
  bool any_bad() const;
  void sum_first_pass();
  void cut_heavy();
  void sort_heavy();
  void settle_lane();
  void fewer_chunks_for_long_chains();
  void chunk_boundaries();
};

// The batch is cut into chunks that are planned, uploaded and launched one after the other: while the GPU runs
// chunk i the host plans the following ones, the big DP launches of consecutive chunks alternate between two streams
// (the next chunk fills the CUs while the previous one drains), launches of a few tasks (each a full task latency
// long) go, longest first, to whichever stream has the least work queued, and the traceback of a chunk runs next to
// the following chunk's DP.  Direction-flag regions rotate over `nreg_ws` slices of the workspace.
// (small batches stay on the caller's stream -- unless they hold long tasks: their launch classes, each as long
// as its longest task, then run side by side on the other streams like those of a large batch)
void Cutter::decide_pipeline(bool pipeline_enabled) {
  bool any_long = false;
  if (n < 2048)
    for (size_t k = 0; k < n && !any_long; ++k) any_long = tasks[k].qlen + (int64_t)tasks[k].tlen >= 3000;
  cut.pipelined = pipeline_enabled && (n >= 2048 || any_long);
  cut.nch = 1;
  // (sixteen or twenty-four chunks for a million tasks were measured no better than eight)
  // (two, three or six chunks for the 100,000-task headline batch: within noise of four)
  if (cut.pipelined && n >= 32768) cut.nch = std::min<size_t>(n >= 500000 ? 8 : 4, n / 16384);
  if (force_nch > 0 && cut.pipelined) cut.nch = (size_t)force_nch;
  cut.max_regions = cut.nch > 4 ? 8 : cut.nch > 1 ? 4 : 1;
  nch_by_size = cut.nch;
  // the first chunk is small, so that the GPU starts early, but fills the wavefront slots of the device (4,096 pairs
  // of tasks of the headline shape) while the next chunks are being planned
  first_target0 = nch_by_size > 1 ? std::max<size_t>(8192, n / (16 * nch_by_size + 1)) : n;
  // (on the context's parked planning threads when there are any; this thread takes a share too)
  // (from 400,000 tasks: on the 100,000-task headline batch four scan threads were measured at 5.2 ms of planning
  // before the first launch against 1.2 ms on this thread alone -- the wake-up of parked threads, not the scan)
  // (the parked threads scan the cut of every batch that has them -- sdf_api.hip: from 120,000 tasks -- : with them the scan
  // runs in two passes and the heavy chunks start after the first, over the big tasks only.  It was 400,000 until round 4:
  // an eighth / a quarter of the hg19 mixture, what a rank of an 8- / 4-GPU strong-scaling run gets, 5.6-5.7 -> 4.9-5.3 ms
  // and 7.2-7.5 -> 5.9-6.0 ms, first launch at 0.56 instead of 1.39 ms.  SDF_SCAN_POOL_FROM overrides.)
  nthr = pool && n >= (size_t)env.cfg->scan_pool_from ? std::min(16, pool->size() + 1) : 1;
}

void Cutter::prepare_scratch() {
  if (lane_scan && cut.lane.size() < n) cut.lane.resize(n);
  // (not cleared: 8 MB of memset per million tasks, on this thread, before anything else can start -- the scan below
  // writes both words of every task, runnable or not)
  if (cut.bound.size() < n) cut.bound.resize(n);
  if (cut.cap.size() < n) cut.cap.resize(n);
  for (auto &hp : cut.hparts) hp.clear();
  for (auto &ht : cut.htasks) ht.clear();
  cut.heavy_tasks.clear();
  cut.blocks.assign(nblk, BatchCut::Block());
}

// what a task needs of the chunks' budgets (task_needs, through the thread's memo) into its block's sums
void Cutter::account(size_t k, Part &pt, std::vector<uint32_t> &hv, const bool may_be_heavy) {
  const sdf_task &t = tasks[k];
  BatchCut::Block &blk = cut.blocks[k / SDF_CUT_BLOCK];
  pt.rows_max = std::max(pt.rows_max, (int64_t)t.qlen + t.tlen);
  Memo &mm = pt.memo[((uint32_t)t.qlen * 31u + (uint32_t)t.tlen * 17u + (uint32_t)t.w) & 255u];
  const int32_t so = t.flag & SDF_FLAG_SCORE_ONLY;
  if (mm.qlen != t.qlen || mm.tlen != t.tlen || mm.w != t.w || mm.so != so) {
    mm.nd = task_needs(env, t);
    mm.qlen = t.qlen, mm.tlen = t.tlen, mm.w = t.w, mm.so = so;
  }
  const TaskNeeds &nd = mm.nd;
  ++blk.nt;
  blk.oc += nd.oc;
  cut.cap[k] = 0x80000000u | nd.words;
  blk.sw += nd.words;
  cut.bound[k] = (uint32_t)std::min<size_t>(nd.bd >> 8, 0xffffffffu);
  blk.bd += (uint64_t)cut.bound[k] << 8;
  if (std::max(nd.bd, nd.hvb) >= heavy_min && may_be_heavy) {
    ++pt.nh;
    pt.hb += nd.bd;
    ++blk.hnt;
    blk.hbd += (uint64_t)cut.bound[k] << 8;
    blk.hsw += nd.words;
    blk.hoc += nd.oc;
    if (pt.nh <= hv_limit) {  // (beyond a quarter of the batch there is no split)
      hv.push_back((uint32_t)k);
      cut.htasks[&hv - &cut.hparts[0]].push_back(t);
    }
  }
}

// a lane task: sixteen bytes for the device and four sums, nothing else
void Cutter::fill_lane(size_t k) {
  const sdf_task &t = tasks[k];
  const bool dir = with_dir(env, t);
  BatchCut::Block &blk = cut.blocks[k / SDF_CUT_BLOCK];
  cut.lane[k] = 1;
  LaneRec &lr = env.lane_recs[k];
  lr.q_word = (uint32_t)t.q_off;
  lr.t_word = (uint32_t)t.t_off;
  lr.out_idx = (uint32_t)k;
  lr.qlen_m1 = (uint8_t)(t.qlen - 1);
  lr.tlen_m1 = (uint8_t)(t.tlen - 1);
  lr.flag = (uint16_t)((t.flag & SDF_FLAG_REV_CIGAR) | (dir ? 0 : SDF_FLAG_SCORE_ONLY));
  ++blk.lnt;
  blk.lsw += dir ? stage_words(t) : 0u;
  blk.ldir += dir ? lane_dir_bytes(t.qlen, t.tlen) : 0;
  ++blk.lcls[lane_class(t.qlen)];
}

// (big: everything a stripe / strip kernel may take -- more than 256 target bases --, and from 40,000 cells or 1,000
// anti-diagonals; the others have two launch-order entries and no direction-flag bound near heavy_min)
bool Cutter::is_big(const sdf_task &t) const {
  return t.tlen > 256 || (int64_t)t.qlen * t.tlen >= 40000 || (int64_t)t.qlen + t.tlen >= 1000 || banded_long(env, t);
}

// mode 0: every task; 1: the big tasks only (and the sums of the early start); 2: the others, none of them heavy
void Cutter::scan(size_t lo, size_t hi, Part &pt, std::vector<uint32_t> &hv, const int mode) {  // (lo: a multiple of the block size)
  for (size_t k = lo; k < hi; ++k) {
    const sdf_task &t = tasks[k];
    if (mode == 1) {
      pt.words += (int64_t)t.qlen + t.tlen + 2;
      if (!is_big(t)) continue;
      ++pt.nbig;
      pt.big_oc += order_entries(env, t);
    } else if (mode == 2 && is_big(t)) {
      continue;
    }
    if (t.flag & ~0xff) {  // (not KSW_EZ_* bits of the extz2 kernel: the splice bits, and everything beyond the KSW_EZ_* range --
                           // the strand bits of a resident task never get here, sdf_api.hip: planner_flag)
      pt.bad = true;
      return;
    }
    cut.bound[k] = 0;
    cut.cap[k] = 0;
    if (lane_scan) {
      cut.lane[k] = 0;
      env.lane_recs[k].flag = 0xffffu;
    }
    if (!task_runs(t, env.degenerate)) continue;
    // the lane kernel's (if the batch turns out to hold enough of them: else these tasks are accounted for in a second
    // pass, settle_lane)
    if (lane_scan && lane_task(t)) fill_lane(k);
    else account(k, pt, hv, mode != 2);
  }
}

// one pass over the batch in `mode` (see scan); `meanwhile`: what this thread does first, while the helpers read
// Runs of sixteen blocks are handed out through a counter: this thread starts at once, a parked helper joins when it
// has woken up (which takes up to milliseconds on a box with a CPU quota) and takes what is left -- nobody waits
// for a share that was dealt to a thread still asleep.
void Cutter::run_pass(const int mode, const std::function<void()> *meanwhile) {
  struct Share {
    std::atomic<size_t> next{0}, done{0};
  };
  const size_t run_blocks = 16, nrun = (nblk + run_blocks - 1) / run_blocks;  // (runs of 1 / 2 / 4 blocks: 3.3-4.0 / 2.0-2.7 / 1.8-2.5 ms
                                                                              // per million tasks against 1.3-2.1)
  auto share = std::make_shared<Share>();  // (outlives this call: a helper may wake up after everything is done)
  auto work = [this, share, nrun, mode](int q) {  // (touches nothing of the cutter once the runs are handed out)
    for (size_t ru = share->next.fetch_add(1); ru < nrun; ru = share->next.fetch_add(1)) {
      if (!parts[q].bad)
        scan(ru * run_blocks * SDF_CUT_BLOCK, std::min(n, (ru + 1) * run_blocks * SDF_CUT_BLOCK), parts[q], cut.hparts[q], mode);
      share->done.fetch_add(1);
    }
  };
  for (int q = 1; q < nthr; ++q) pool->submit([work, q] { work(q); });
  if (meanwhile) (*meanwhile)();
  work(0);
  while (share->done.load() < nrun) std::this_thread::yield();  // (a helper still inside its last run)
}

bool Cutter::any_bad() const {
  for (int q = 0; q < nthr; ++q)
    if (parts[q].bad) return true;
  return false;
}

// after the pass over the big tasks: the upper bounds the early start sizes its buffers by
void Cutter::sum_first_pass() {
  size_t nbig = 0, big_oc = 0;
  for (int q = 0; q < nthr; ++q) {
    cut.stage_upper += parts[q].words;
    nbig += parts[q].nbig;
    big_oc += parts[q].big_oc;
  }
  cut.order_upper = big_oc + 2 * (n - nbig) + 64;
}

// (the scan threads took their runs of blocks in any order: sorted by task index, the records along)
void Cutter::sort_heavy() {
  std::vector<std::pair<uint32_t, uint32_t>> by_idx;  // (task, position in the concatenation of the threads' lists)
  std::vector<const sdf_task *> rec;
  for (int q = 0; q < 16; ++q)
    for (size_t j = 0; j < cut.hparts[q].size(); ++j) {
      by_idx.push_back({cut.hparts[q][j], (uint32_t)rec.size()});
      rec.push_back(&cut.htasks[q][j]);
    }
  std::sort(by_idx.begin(), by_idx.end());
  cut.heavy_idx.resize(by_idx.size());
  cut.heavy_tasks.resize(by_idx.size());
  for (size_t j = 0; j < by_idx.size(); ++j) {
    cut.heavy_idx[j] = by_idx[j].first;
    cut.heavy_tasks[j] = *rec[by_idx[j].second];
  }
}

// Heavy tasks leave the chunk rotation when they are a minority: they are planned and launched FIRST, all together
// (a launch of few long tasks lasts as long as its longest task: one such launch per kernel, not one per chunk), with
// a workspace slice of their own, and run next to the chunks of ordinary tasks.
void Cutter::cut_heavy() {  // (after the pass that finds them)
  for (int q = 0; q < nthr; ++q) {
    cut.n_heavy += parts[q].nh;
    heavy_bytes += parts[q].hb;
  }
  cut.split_heavy = cut.pipelined && cut.n_heavy * 4 <= n;
  heavy_budget = cut.split_heavy && cut.n_heavy ? std::min(heavy_bytes + 256, ws_budget / 2) : 0;
  // (round 6) a batch whose flags fit the workspace as a whole: the heavy tasks take what they need in ONE chunk -- a
  // launch of few long tasks lasts as long as its longest chain however the rest is cut -- and the others the rest.  Known
  // only where the scan has seen every task (the single pass of a batch below the two-pass threshold).
  if (heavy_budget && !two_pass && heavy_bytes + 256 > heavy_budget) {
    uint64_t all = 0;
    for (const BatchCut::Block &blk : cut.blocks) all += blk.bd;
    const double rest = (double)(all - std::min<uint64_t>(all, heavy_bytes)) * 1.05 + 4096.0;
    if ((double)heavy_bytes + 256 + rest + (double)cut.lane_dir_bytes <= (double)ws_budget) heavy_budget = heavy_bytes + 256;
  }
  cut.heavy.assign(cut.split_heavy ? n : 0, 0);
  if (!cut.split_heavy) return;
  sort_heavy();
  // heavy chunks: ranges of the (ascending) list of heavy tasks
  ChunkPlan hcur;
  hcur.heavy = true;
  size_t hacc = 0;
  for (size_t pos = 0; pos < cut.heavy_idx.size(); ++pos) {
    if (pos + 16 < cut.heavy_idx.size()) {  // (the heavy tasks lie scattered over the batch: a cache miss each)
      const uint32_t kn = cut.heavy_idx[pos + 16];
      __builtin_prefetch(&cut.bound[kn]);
      __builtin_prefetch(&cut.cap[kn]);
    }
    const uint32_t k = cut.heavy_idx[pos];
    const size_t bd = (size_t)cut.bound[k] << 8;
    cut.heavy[k] = 1;
    if (pos > hcur.s && hacc + bd > heavy_budget) {
      hcur.e = pos;
      heavy_chunks.push_back(hcur);
      cut.heavy_need = std::max(cut.heavy_need, hacc);
      hcur = ChunkPlan();
      hcur.heavy = true;
      hcur.s = pos;
      hacc = 0;
    }
    hacc += bd;
    ++hcur.ntask;
    hcur.stage_words += cut.cap[k] & 0x7fffffffu;
    hcur.order_cap += order_entries(env, cut.heavy_tasks[pos]);
  }
  if (!cut.heavy_idx.empty()) {
    hcur.e = cut.heavy_idx.size();
    heavy_chunks.push_back(hcur);
    cut.heavy_need = std::max(cut.heavy_need, hacc);
  }
  cut.heavy_need = round256(cut.heavy_need);
}

// the lane tasks' sums; too few of them after all: they are ordinary tasks
void Cutter::settle_lane() {
  for (const BatchCut::Block &blk : cut.blocks) {
    cut.n_lane += blk.lnt;
    cut.lane_stage_words += blk.lsw;
    cut.lane_dir_bytes += blk.ldir;
    for (int c = 0; c < 4; ++c) cut.lane_cls[c] += blk.lcls[c];
  }
  // (a quarter of the workspace in 4-bit flags would be more than 10^10 cells of small tasks)
  cut.use_lane = cut.n_lane >= (size_t)env.cfg->lane_min && cut.lane_dir_bytes + 256 <= ws_budget / 4;
  if (cut.use_lane || !cut.n_lane) return;
  for (size_t k = 0; k < n; ++k)
    if (cut.lane[k]) {
      cut.lane[k] = 0;
      account(k, parts[0], cut.hparts[0], !two_pass);
    }
  cut.n_lane = 0;
}

// A launch lasts as long as its longest task -- a chain of qlen + tlen dependent rows, ~0.5 us each when the wavefront
// shares its SIMD -- whatever else runs: a chunk whose whole work is a few such chains long keeps the device waiting
// for one wavefront at the end of each of its launches (a batch of banded tasks of all lengths, BASELINE configs[4]:
// fourteen chunks 400-580 ms, one chunk 220 ms, profiles/r04_shapes.txt).  Such a batch is cut into fewer chunks:
// each at least six chains' worth of work (the bytes of the direction flags stand for the cells: ~0.65 B each at a
// Tcell/s), the workspace permitting.
void Cutter::fewer_chunks_for_long_chains() {
  if (two_pass || cut.split_heavy || cut.nch <= 1 || force_nch) return;
  int64_t rows_max = 0;
  uint64_t bytes = 0;
  for (int q = 0; q < nthr; ++q) rows_max = std::max(rows_max, parts[q].rows_max);
  for (const BatchCut::Block &blk : cut.blocks) bytes += blk.bd;
  const double chain_ms = (double)rows_max * 0.5e-3, work_ms = (double)bytes / 0.65e9;
  const size_t nch_max = (size_t)std::max(1.0, work_ms / (6.0 * chain_ms));
  if (nch_max >= cut.nch) return;
  // (no small first chunk either: it would hold a whole region of the workspace for a twelfth of the tasks, and the
  // planning it hides is a few milliseconds of a call of hundreds)
  // Chunks of equal task counts, a workspace region each while the flags of the whole batch fit the workspace; beyond
  // that two regions, the chunks as large as a region holds (two in flight, the third waits for the first's walk).
  const size_t avail = ws_budget - std::min(ws_budget / 2, (size_t)cut.lane_dir_bytes);
  const double need = (double)bytes * 1.05;
  if (need <= (double)avail) {
    cut.nch = nch_max;
    cut.max_regions = std::max<size_t>(1, cut.nch);
  } else {
    cut.max_regions = 2;
    cut.nch = std::max<size_t>(2, (size_t)(need / ((double)avail / 2.0)) + 1);
  }
  chain_bound = true;
}

// whole blocks of tasks at a time (their sums come from the scan); task by task only inside a block that
// does not fit the region as a whole
void Cutter::chunk_boundaries() {
  const size_t lane_budget = cut.use_lane ? cut.lane_dir_bytes + 256 : 0;
  const size_t region_budget = (ws_budget - heavy_budget - lane_budget) / cut.max_regions;
  const size_t nch = cut.nch;
  const size_t first_target = chain_bound ? (n + nch - 1) / nch : nch_by_size > 1 ? first_target0 : n;
  const size_t chunk_target = chain_bound ? (n + nch - 1) / nch : nch_by_size > 1 ? (n - first_target + nch - 1) / nch : n;
  std::vector<ChunkPlan> normal;
  ChunkPlan cur;
  size_t acc = 0;
  const uint8_t *hv = cut.split_heavy ? cut.heavy.data() : nullptr;
  const uint8_t *ln = cut.use_lane ? cut.lane.data() : nullptr;
  auto close_at = [&](size_t k) {
    cur.e = k;
    normal.push_back(cur);
    cut.region_need = std::max(cut.region_need, acc);
    cur = ChunkPlan();
    cur.s = k;
    acc = 0;
  };
  for (size_t b = 0; b < nblk; ++b) {
    const size_t k0 = b * SDF_CUT_BLOCK, k1 = std::min(n, k0 + SDF_CUT_BLOCK);
    const BatchCut::Block &blk = cut.blocks[b];
    const size_t target = normal.empty() && nch_by_size > 1 ? first_target : chunk_target;
    // (all tasks of the range count towards the target, as they cost planning time whether they run or not)
    if (k0 > cur.s && k0 - cur.s >= target) close_at(k0);
    const uint64_t bbd = blk.bd - (hv ? blk.hbd : 0);  // (lane tasks are not in a block's sums)
    if (acc + bbd <= region_budget) {
      acc += bbd;
      cur.ntask += blk.nt - (hv ? blk.hnt : 0);
      cur.stage_words += blk.sw - (hv ? blk.hsw : 0);
      cur.order_cap += blk.oc - (hv ? blk.hoc : 0);
      continue;
    }
    for (size_t k = k0; k < k1; ++k) {
      if (hv && hv[k]) continue;
      if (ln && ln[k]) continue;
      const size_t bd = (size_t)cut.bound[k] << 8;
      if (k > cur.s && acc + bd > region_budget) close_at(k);
      acc += bd;
      cur.ntask += cut.cap[k] >> 31;
      cur.stage_words += cut.cap[k] & 0x7fffffffu;
      cur.order_cap += (cut.cap[k] >> 31) * order_entries(env, tasks[k]);
    }
  }
  close_at(n);
  cut.region_need = round256(cut.region_need);
  cut.heavy_need = round256(cut.heavy_need);
  cut.nreg_ws = std::min(cut.max_regions, normal.size());
  cut.chunks = heavy_chunks;  // heavy first
  cut.chunks.insert(cut.chunks.end(), normal.begin(), normal.end());
}

}  // namespace

// Returns SDF_OK or an error code with *err set.
// `early` (optional): called once the heavy chunks are known -- cut.chunks holds them, with their bases; cut.heavy_need,
// stage_upper, order_upper are set -- while the rest of the batch is still being read: it plans and launches them and
// sets cut.n_early (batches of 400,000 tasks and more on a context with planning threads: the long tasks of a batch are
// the launch that ends it, and the pass over a million task records is 1-2 ms it need not wait for).
int cut_batch(const PlanEnv &env, bool pipeline_enabled, size_t ws_budget, BatchCut &cut, const char **err, WorkerPool *pool,
              const std::function<int()> *early) {
  const auto tc0 = std::chrono::steady_clock::now();
  Cutter cu(env, cut, ws_budget, pool);
  cu.decide_pipeline(pipeline_enabled);
  cu.prepare_scratch();
  // ---- validation + upper bound of each task's direction flags, whichever kernel takes it ----
  // (on several threads for batches of hundreds of thousands of tasks: this pass and the boundaries are all the
  // planning the GPU waits for besides the first chunk)
  cu.two_pass = early && *early && cu.nthr > 1 && cut.pipelined;
  int early_rc = SDF_OK;
  if (cu.two_pass) {
    cu.run_pass(1, nullptr);
    if (cu.any_bad()) {
      *err = "unknown task flag";
      return SDF_ERR_UNSUPPORTED;
    }
    cu.sum_first_pass();
    cu.cut_heavy();
    for (int q = 0; q < cu.nthr; ++q) cu.parts[q].nh = cu.parts[q].hb = 0;
    const std::function<void()> start = [&]() {
      if (!cut.split_heavy || cu.heavy_chunks.empty()) return;
      cut.chunks = cu.heavy_chunks;  // (their bases: heavy chunks come first)
      assign_bases(cut, false);
      early_rc = (*early)();
      for (size_t q = 0; q < cu.heavy_chunks.size() && q < cut.chunks.size(); ++q) cu.heavy_chunks[q] = cut.chunks[q];  // (planned)
    };
    cu.run_pass(2, &start);
  } else {
    cu.run_pass(0, nullptr);
  }
  if (early_rc != SDF_OK) {
    *err = "early start of the heavy chunks failed";
    return early_rc;
  }
  if (cu.lane_scan) cu.settle_lane();
  if (cu.any_bad()) {
    *err = "unknown task flag";
    return SDF_ERR_UNSUPPORTED;
  }
  if (!cu.two_pass) cu.cut_heavy();
  cu.fewer_chunks_for_long_chains();
  const auto tc1 = std::chrono::steady_clock::now();
  cu.chunk_boundaries();
  assign_bases(cut, true);
  if (env.cfg->debug_plan != 0 && env.n >= 100000)
    fprintf(stderr, "[cut: clear + scan %.2f ms, boundaries %.2f ms]\n", std::chrono::duration<double, std::milli>(tc1 - tc0).count(),
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tc1).count());
  return SDF_OK;
}

// ---- plan_chunk: its passes ---------------------------------------------------------------------------------------------
namespace {
using Family = LaunchClass::Family;

// Which task does position `pos` of a chunk mean: a heavy chunk lists cut.heavy_idx (the records in the compact copy), an
// ordinary one the caller's array minus its heavy tasks.  f(k, t) for each.
template <class F>
void for_each_task(const PlanEnv &env, const BatchCut &cut, const ChunkPlan &c, F f) {
  for (size_t pos = c.s; pos < c.e; ++pos) {
    const size_t k = c.heavy ? cut.heavy_idx[pos] : pos;
    if (!c.heavy && cut.split_heavy && cut.heavy[k]) continue;
    f(k, c.heavy ? cut.heavy_tasks[pos] : env.tasks[k]);
  }
}

struct Chunk {
  const PlanEnv &env;
  const BatchCut &cut;
  ChunkPlan &c;
  PlanTask *const cp;  // the chunk's tasks: chunk-relative indexing
  int32_t *const order;
  PlanScratch &sx;
  std::vector<int32_t> &win_need = sx.win_need, &partner = sx.partner;
  std::vector<char> &mixedf = sx.mixedf, &tracked = sx.tracked;
  std::vector<std::pair<int32_t, int32_t>> &table = sx.table;
  std::vector<Cls> &cls = sx.cls;
  size_t cnt = 0;
  bool use_strip = false, use_chain = false, long_to_stripes = false, use_mixed = false;
  size_t n_stripe_tasks = 0;   // stripe tasks of the chunk,
  double stripe_cells = 0;     // their cells,
  int stripe_rows = 0;         // the anti-diagonals of the longest of them

  void strips_or_not();
  PlanTask choose_kind(size_t k, const sdf_task &t, int &wneed, int (&bs_alt)[2]) const;
  void choose_kinds();
  void stripe_width();
  void mixed_or_not();
  void pair_exact();
  void add_mix_key(size_t k);
  void pair_mixed();
  void pair_self();
  void chain_columns();
  void sort_strip_keys();
  void pair_strips();
  bool layout_and_classes();
  void merge_classes();
  void longest_first_in_class();
  bool deal_stripes(const Cls &x, size_t &cursor);
  void launch_order();
};

// Strip kernels (extz2_strip.hip) are throughput kernels: a step of eight cells per lane is a microsecond on a wavefront
// alone, a 500 x 500 task 0.55 ms where the window kernels take 0.3, a chain of twelve blocks 6.5 ms against the
// stripe kernel's 3.0 (profiles/r03_strip.txt).  They take a chunk's tasks only when there are enough of them to fill
// the device: 1,024 one-wavefront tasks, 3,072 chain wavefronts (1,024 for the heavy tasks of a large batch).
void Chunk::strips_or_not() {
  if (env.strip_ok) {
    const bool force = env.cfg->strip_always != 0;  // (tests: whatever the count)
    size_t n9 = 0, w10 = 0;
    for_each_task(env, cut, c, [&](size_t, const sdf_task &t) {
      if (!(strip_range(t) || chain_range(t)) || t.qlen < 64 || !full_band(t)) return;
      if (strip_range(t)) ++n9;
      else w10 += (size_t)strip_blocks(t.tlen, 8);
    });
    use_strip = force || n9 >= 1024;
    // (the heavy tasks of a large batch share the device with everything else it holds: what counts there is the work per
    // cell, not the pace of a lone chain -- the hg19 mixture's 608 long tasks, 2,900 chain wavefronts: 13.5-14.0 ms as chains
    // against 14.2-15.2 on the stripe kernel; the same tasks alone: 10-15 % slower as chains)
    const size_t chain_min = c.heavy && cut.n_heavy * 16 <= env.n ? std::min<size_t>((size_t)env.cfg->chain_min, 1024) : (size_t)env.cfg->chain_min;
    use_chain = force || w10 / 2 >= chain_min;
  }
  // (a few tasks much longer than the rest of a chunk of chains take the stripe kernel: sdf_plan_rules.h, long_task)
  size_t n_long = 0;
  if (use_chain && !env.cfg->strip_always && !env.cfg->no_stripe)
    for_each_task(env, cut, c, [&](size_t, const sdf_task &t) { n_long += long_task(env, t); });
  long_to_stripes = n_long > 0 && n_long <= 64;
}

// One task: the kernel that takes it (p.kind, p.nreg), the window it needs on the wave / pair kernels (wneed, 0: none) and,
// for a task given to the banded stripe kernel that a mixed pair could take, the wave registers and window (bs_alt).
// A stripe task's width and a chain's columns are its chunk's: decided after this pass.
PlanTask Chunk::choose_kind(const size_t k, const sdf_task &t, int &wneed, int (&bs_alt)[2]) const {
  PlanTask p;
  p.q_word = t.q_off;
  p.t_word = t.t_off;
  p.qlen = t.qlen;
  p.tlen = t.tlen;
  p.w = resolved_w(t);
  p.zdrop = t.zdrop;
  p.flag = t.flag | (env.want_cigar() ? 0 : SDF_FLAG_SCORE_ONLY);
  p.ncol16 = ncol16(t);
  p.out_idx = (int32_t)k;
  p.kind = kTaskGeneral;
  // register-resident wave kernel when only CIGAR/score/mte are wanted and the shape fits
  p.nreg = 0;
  p.dir_off = 0;
  p.cig_cap = (p.flag & SDF_FLAG_SCORE_ONLY) ? 0 : (int32_t)stage_words(t);
  p.cig_slot = 0;
  wneed = bs_alt[0] = bs_alt[1] = 0;
  const int need = window_need(t);
  const bool whole = band_whole(t);
  const bool plain_ok = simple(env, t) && whole && !env.force_general;
  if (bstripe_wanted(env, t, whole)) {
    const int nr = bstripe_nreg(t.tlen, (int)env.cfg->bstripe_nreg);
    if (nr && bstripe_lds_bytes(p.w, nr) <= (size_t)env.max_dyn_lds) {
      p.nreg = nr;
      p.kind = kTaskBStripe;
      if (plain_ok && need <= kMixedMaxNeed && !env.cfg->no_pair && !env.cfg->no_mixed &&  // (band_whole: a mixed pair can take it)
          wave_lds_bytes(t.qlen, t.tlen, wave_nreg(need)) <= (size_t)env.max_dyn_lds) {
        bs_alt[0] = wave_nreg(need);
        bs_alt[1] = need;
      }
    }
  }
  // the same request on a band that runs out before the end of both sequences: the pair kernel's TRACK flavour
  // (exact H of every cell, best cell for the traceback), the task paired with itself; windows up to 384 slots
  const bool runs_out = !whole && p.w >= 1 && t.qlen + t.tlen - 1 > 1;
  if (p.kind != kTaskBStripe && runs_out && !env.force_general && !env.cfg->no_pair && simple(env, t)) {
    const int nreg = track_nreg(need);
    if (nreg && pair_lds_bytes(t.qlen, t.tlen, nreg) <= (size_t)env.max_dyn_lds) {
      p.nreg = nreg;
      p.kind = kTaskTrack;  // (a kTaskPair paired with itself below; marks the TRACK launch class until then)
    }
  }
  if (plain_ok && p.kind != kTaskBStripe) {
    const int nreg = wave_nreg(need);
    if (nreg && wave_lds_bytes(t.qlen, t.tlen, nreg) <= (size_t)env.max_dyn_lds) {
      p.nreg = nreg;
      wneed = need;
    }
  }
  const bool full_plain = p.kind != kTaskBStripe && plain_ok && full_band(t);
  if (use_strip && full_plain && strip_range(t) && strip_rows(t)) {
    // full band, a few hundred target bases: row-major strips, two tasks per wavefront
    p.nreg = 8;  // (columns per lane)
    p.kind = kTaskStrip;
    wneed = 0;
  } else if ((use_chain || (env.strip_ok && t.tlen > kStripeMaxT)) && !(long_to_stripes && long_task(env, t)) && !env.cfg->no_stripe &&
             full_plain && chain_range(t) && strip_rows(t)) {
    // ... wider: the same strips, a wavefront per block of columns, chained through HBM.  Targets beyond the stripe
    // kernel's 32,512 bases are chains however few they are: the alternative is the workgroup kernel walking its window
    // through LDS at ~3 us per row (a 61,440 x 61,440 task alone: 2,070 ms there, 80 ms here)
    p.nreg = 8;  // (columns per lane: 8, or 4 when the chunk has few chains -- chain_columns)
    p.kind = kTaskChain;
    wneed = 0;
  } else if (full_plain && !env.cfg->no_stripe && stripe_range(env, t)) {
    // wide full-band task: one wavefront per stripe of 128 * nreg target positions (nreg: stripe_width)
    if (stripe_lds_ok(env, t)) {
      p.nreg = 4;
      p.kind = kTaskStripe;
    }
  }
  if (!p.nreg) {
    // general kernel: state in LDS, or in an HBM scratch slab when it does not fit; the PLAIN flavour (packed
    // recurrence, H along the band edge only) when nothing but CIGAR / score / mte is wanted and the window
    // is wide enough for the 256- or 1024-thread instantiation
    const bool hbm = general_lds_bytes(t.qlen, t.tlen) > (size_t)env.max_dyn_lds;
    const int width = general_width(p.ncol16, t.tlen);
    if (plain_ok && !hbm && width > 256) p.kind = kTaskPlain;
    else if (plain_ok && hbm && width > 1024) p.kind = kTaskPlainHbm;
    else p.kind = hbm ? kTaskGeneralHbm : kTaskGeneral;
  }
  return p;
}

void Chunk::choose_kinds() {
  win_need.clear();
  sx.bs_alt.clear();
  int64_t stage = c.stage0;
  for_each_task(env, cut, c, [&](size_t k, const sdf_task &t) {
    if (cut.use_lane && cut.lane[k]) return;  // (planned on the device: extz2_lane.hip)
    if (!task_runs(t, env.degenerate)) return;  // reference early return (:57,:81)
    int wneed, alt[2];
    PlanTask p = choose_kind(k, t, wneed, alt);
    if (alt[0]) sx.bs_alt.insert(sx.bs_alt.end(), {(int32_t)cnt, alt[0], alt[1]});
    win_need.push_back(wneed);
    p.cig_slot = stage;
    stage += p.cig_cap;
    if (p.kind == kTaskStripe) {
      ++n_stripe_tasks;
      stripe_cells += (double)t.qlen * (double)t.tlen;
      stripe_rows = std::max(stripe_rows, t.qlen + t.tlen);
    }
    cp[cnt++] = p;
  });
}

// One stripe width per chunk (one launch, all its tasks side by side).  A wavefront alone on its SIMD issues an
// instruction every ~5 cycles whatever its width, so a row of a 128-position stripe takes a quarter of the time of
// a row of a 512-position one, and a task is a chain of qlen + tlen dependent rows: few tasks want narrow stripes
// (a 6000 x 6000 task alone: 6.1 ms at 512 positions per stripe).  Many tasks want wide ones: per cell a wide stripe
// spends fewer instructions on the edges and the loop (1k x 1k tasks by the thousand: 1180 Gcell/s at 512, 800 at
// 128), and with a wavefront or more per SIMD the chains overlap anyway.
void Chunk::stripe_width() {
  const int force_nreg = (int)env.cfg->stripe_nreg;
  // -> the width with the smaller of: the launch's cells at the width's throughput (800 / 1100 / 1300 Gcell/s measured
  // on batches of equal tasks), its longest chain at the width's row time alone on a SIMD (0.24 / 0.27 / 0.50 us)
  int nr = 1;
  {
    const double rate[3] = {800e3, 1100e3, 1300e3}, row_us[3] = {0.24, 0.27, 0.50};  // cells per us; us per row
    double best = 1e300;
    for (int q = 0; q < 3; ++q) {
      const double t_us = std::max(stripe_cells / rate[q], (double)stripe_rows * row_us[q]);
      if (t_us < best) {
        best = t_us;
        nr = 1 << q;
      }
    }
    if (force_nreg) nr = force_nreg;
  }
  for (size_t k = 0; k < cnt; ++k) {
    PlanTask &p = cp[k];
    if (p.kind != kTaskStripe) continue;
    p.nreg = nr;
    if ((p.tlen + 128 * nr - 1) / (128 * nr) > 254) {  // (entry encoding: 8 bits of stripe index, 255 = idle)
      p.nreg = 0;
      const bool hbm = general_lds_bytes(p.qlen, p.tlen) > (size_t)env.max_dyn_lds;
      p.kind = hbm ? kTaskPlainHbm : kTaskPlain;
    }
  }
}

// Mixed pairs are a throughput kernel (a wavefront of nine registers takes ~1.3 us per row when it shares its SIMD): the
// chunk's banded tasks take them when there are enough to fill the device, and then the long ones whose band reaches the
// end come back from the banded stripe kernel (0.73 VALU instructions per cell measured there against ~0.4-0.5 here,
// profiles/r04_mm8_pmc.txt); in a chunk of few tasks a long task stays a chain of short stripe rows.
void Chunk::mixed_or_not() {
  mixedf.assign(cnt, 0);
  if (env.cfg->no_pair || env.cfg->no_mixed || env.force_general) return;
  size_t ncand = sx.bs_alt.size() / 3;
  for (size_t k = 0; k < cnt; ++k)
    ncand += cp[k].nreg && cp[k].kind == kTaskGeneral && win_need[k] > 0 && win_need[k] <= kMixedMaxNeed && !full_band(cp[k]);
  use_mixed = ncand >= (size_t)env.cfg->mixed_min;
  if (use_mixed)
    for (size_t j = 0; j + 2 < sx.bs_alt.size(); j += 3) {
      PlanTask &p = cp[sx.bs_alt[j]];
      p.kind = kTaskGeneral;
      p.nreg = sx.bs_alt[j + 1];
      win_need[sx.bs_alt[j]] = sx.bs_alt[j + 2];
    }
}

// Pair kernel: two wave-eligible tasks of the chunk with the same (qlen, tlen, w, flag) and a window of at
// most 512 slots share a wavefront (extz2_pair.hip).  partner[k] = the other task, or -1.  One pass with an
// open-addressing table keyed by the geometry: entry = (first task seen with the key, the task of that key
// still waiting for a partner or -1).
void Chunk::pair_exact() {
  size_t cap = 64;
  while (cap < 2 * cnt) cap *= 2;
  table.assign(cap, {-1, -1});
  for (size_t k = 0; k < cnt; ++k) {
    PlanTask &y = cp[k];
    if (!y.nreg || y.kind != kTaskGeneral || win_need[k] > 512) continue;  // wave-kernel tasks only
    uint64_t h = ((uint64_t)(uint32_t)y.qlen * 0x9E3779B97F4A7C15ull) ^ ((uint64_t)(uint32_t)y.tlen * 0xC2B2AE3D27D4EB4Full) ^
                 ((uint64_t)(uint32_t)y.w * 0x165667B19E3779F9ull) ^ ((uint64_t)(uint32_t)y.flag << 40);
    h ^= h >> 29;
    for (size_t slot = (size_t)h & (cap - 1);; slot = (slot + 1) & (cap - 1)) {
      auto &e = table[slot];
      if (e.first < 0) {
        e = {(int32_t)k, (int32_t)k};
        break;
      }
      const PlanTask &x = cp[e.first];
      if (x.qlen != y.qlen || x.tlen != y.tlen || x.w != y.w || x.flag != y.flag) continue;
      if (e.second < 0) {
        e.second = (int32_t)k;
        break;
      }
      PlanTask &z = cp[e.second];
      const int nreg = pair_nreg(win_need[k]);
      if (pair_lds_bytes(y.qlen, y.tlen, nreg) > (size_t)env.max_dyn_lds) break;
      z.nreg = y.nreg = nreg;
      z.kind = y.kind = kTaskPair;
      partner[k] = e.second;
      partner[e.second] = (int32_t)k;
      c.paired += 2;
      e.second = -1;
      break;
    }
  }
}

void Chunk::add_mix_key(size_t k) {
    const PlanTask &y = cp[k];
    if (full_band(y) || y.w >= (1 << 14) || (y.flag & ~0xff) || k >= ((size_t)1 << 22)) return;
    int cf = pair_clip_free(y.qlen, y.tlen, y.w);
    cf = cf < 0 ? 0 : cf > 0xfffff ? 0xfffff : cf;
    sx.mix_keys.push_back(((uint64_t)(uint32_t)y.w << 50) | ((uint64_t)(uint32_t)(y.flag & 0xff) << 42) | ((uint64_t)cf << 22) | (uint64_t)k);
}

// Mixed pairs: the tasks without a partner of their geometry (and those whose window of 513..576 slots no other pair
// kernel holds), sorted by (w, flag, last clip-free row): neighbours share the most rows.  Worth it when the shared
// rows are at least half of the longer task's (a row of a pair costs ~1.3 rows of the one-task wave kernel).
void Chunk::pair_mixed() {
  std::vector<uint64_t> &keys = sx.mix_keys;
  keys.clear();
  for (auto &e : table)
    if (e.second >= 0) add_mix_key((size_t)e.second);
  for (size_t k = 0; k < cnt; ++k)
    if (cp[k].nreg && cp[k].kind == kTaskGeneral && win_need[k] > 512 && win_need[k] <= kMixedMaxNeed) add_mix_key(k);
  // (a batch of few geometries -- the headline's 100,000 tasks of ~50 target lengths -- leaves a handful without a
  // partner: they are paired with themselves inside the tuned launch, as before, not given a launch of their own)
  if (keys.size() * 16 < cnt) keys.clear();
  std::sort(keys.begin(), keys.end());
  for (size_t q = 0; q + 1 < keys.size();) {
    const size_t a = (size_t)(keys[q] & 0x3fffffu), b = (size_t)(keys[q + 1] & 0x3fffffu);
    PlanTask &x = cp[a], &y = cp[b];
    bool ok = (keys[q] >> 42) == (keys[q + 1] >> 42);  // same band and flags
    int nreg = 0;
    if (ok) {
      const int shared = (x.qlen == y.qlen && x.tlen == y.tlen) ? x.qlen + x.tlen : pair_shared_rows(x.qlen, x.tlen, y.qlen, y.tlen, x.w);
      ok = 2 * shared >= std::max(x.qlen + x.tlen, y.qlen + y.tlen);
      nreg = mixed_nreg(std::max(win_need[a], win_need[b]));
      ok = ok && pair_mixed_lds_bytes(std::max(x.qlen, y.qlen), std::max(x.tlen, y.tlen), nreg) <= (size_t)env.max_dyn_lds;
    }
    if (!ok) {
      ++q;
      continue;
    }
    x.nreg = y.nreg = nreg;
    x.kind = y.kind = kTaskPair;
    partner[a] = (int32_t)b;
    partner[b] = (int32_t)a;
    mixedf[a] = mixedf[b] = 1;
    c.paired += 2;
    q += 2;
  }
  // ... and what is left of them: a long task alone would be a launch of its own on the one-task kernels, as long as its
  // chain of rows; paired with itself it is one more wavefront of the mixed launch (a short one keeps its old routes)
  size_t n_mixed = 0;
  for (size_t q = 0; q < keys.size(); ++q) {
    const size_t a = (size_t)(keys[q] & 0x3fffffu);
    if (partner[a] >= 0) {
      ++n_mixed;
      continue;
    }
    PlanTask &x = cp[a];
    if (x.qlen + x.tlen < 2000) continue;
    const int nreg = mixed_nreg(win_need[a]);
    if (pair_mixed_lds_bytes(x.qlen, x.tlen, nreg) > (size_t)env.max_dyn_lds) continue;
    x.nreg = nreg;
    x.kind = kTaskPair;
    partner[a] = (int32_t)a;
    mixedf[a] = 1;
  }
  // pairs of equal geometry among the banded tasks join the mixed launches when they are the few (a batch of tasks of all
  // lengths: one launch fewer per register count, each as long as its longest chain); a batch of few geometries keeps
  // its tuned instantiations
  size_t n_exact = 0;
  for (size_t k = 0; k < cnt; ++k)
    n_exact += cp[k].kind == kTaskPair && !mixedf[k] && !tracked[k] && partner[k] >= 0 && partner[k] != (int32_t)k && !full_band(cp[k]);
  if (n_exact * 4 <= n_mixed)
    for (size_t k = 0; k < cnt; ++k) {
      PlanTask &x = cp[k];
      if (x.kind != kTaskPair || mixedf[k] || tracked[k] || partner[k] <= (int32_t)k || full_band(x)) continue;
      const int nreg = mixed_nreg(win_need[k]);
      if (pair_mixed_lds_bytes(x.qlen, x.tlen, nreg) > (size_t)env.max_dyn_lds) continue;
      x.nreg = cp[partner[k]].nreg = nreg;
      mixedf[k] = mixedf[partner[k]] = 1;
    }
  for (auto &e : table)  // (no longer waiting)
    if (e.second >= 0 && partner[e.second] >= 0) e.second = -1;
  // a long task that came over from the banded stripe kernel and found nobody goes back to it
  for (size_t j = 0; j + 2 < sx.bs_alt.size(); j += 3) {
    const int32_t k = sx.bs_alt[j];
    if (partner[k] >= 0) continue;
    cp[k].kind = kTaskBStripe;
    cp[k].nreg = bstripe_nreg(cp[k].tlen, (int)env.cfg->bstripe_nreg);
    win_need[k] = 0;
    for (auto &e : table)
      if (e.second == k) e.second = -1;
  }
}

// a task left without a partner is paired with itself (both halves compute the same task and write the
// same bytes) instead of occupying a launch of its own for a whole task latency -- when they are few.  Many of them
// (a batch of banded tasks of all lengths: BASELINE configs[4]) fill launches of their own on the one-task wave
// kernel, whose row is 30-40 % shorter than that of a wavefront whose halves compute the same thing.
void Chunk::pair_self() {
  size_t n_left = 0;
  for (auto &e : table) n_left += e.second >= 0;
  for (auto &e : table) {
    if (e.second < 0 || n_left > (size_t)env.cfg->self_pair_max) continue;
    PlanTask &y = cp[e.second];
    const int nreg = pair_nreg(win_need[e.second]);
    if (pair_lds_bytes(y.qlen, y.tlen, nreg) > (size_t)env.max_dyn_lds) continue;
    y.nreg = nreg;
    y.kind = kTaskPair;
    partner[e.second] = e.second;
  }
}

// Chains: a wavefront alone on its SIMD issues an instruction every ~7 cycles whatever it does, a chain of blocks runs
// at the pace of its steps, and a step of four columns is half as long as one of eight: few chains (the few long
// tasks of a batch: fewer wavefronts than the device has slots for) take four columns per lane, many take eight
// (less per-step overhead per cell).  One width per chunk: one launch.
void Chunk::chain_columns() {
  const int force_cols = (int)env.cfg->strip_cols;
  size_t chain_waves = 0;
  for (size_t k = 0; k < cnt; ++k)
    if (cp[k].kind == kTaskChain) chain_waves += (size_t)strip_blocks(cp[k].tlen, 8);
  // (measured, profiles/r03_strip.txt: four columns shorten a lone chain -- 5.3 against 6.5 ms for 6000 x 6000 -- but
  // cost throughput -- 1,364 against 1,612 Gcell/s on 20,000 x 1000 x 1000 --, and lone chains are the stripe
  // kernel's anyway: eight unless SDF_STRIP_COLS says otherwise)
  // (round 4: a chunk whose chains leave the SIMDs with fewer than four of their wavefronts each takes four -- the heavy
  // chunk of the hg19 mixture, 608 long tasks = 2,900 wavefronts of eight columns: 14.0-14.2 against 14.65-14.85 ms for the
  // 1,000,000-task batch, its DP 9.3-10.8 against 11.6-11.9 ms)
  const int cols = force_cols == 4 || force_cols == 8 ? force_cols : chain_waves / 2 <= 4096 ? 4 : 8;  // (two tasks a wavefront)
  for (size_t k = 0; k < cnt; ++k)
    if (cp[k].kind == kTaskChain) cp[k].nreg = cols;
}

// (8,747 keys in the heavy chunk of the hg19 mixture, planned in front of the call's first launch: a byte-wise radix
// sort over the bytes that differ takes 0.05 ms where std::sort takes 0.25)
void Chunk::sort_strip_keys() {
  std::vector<uint64_t> &keys = sx.strip_keys;
  if (keys.size() >= 2048) {
    std::vector<uint64_t> &tmp = sx.strip_keys_tmp;
    tmp.resize(keys.size());
    uint64_t all_or = 0, all_and = ~0ull;
    for (uint64_t kx : keys) {
      all_or |= kx;
      all_and &= kx;
    }
    const uint64_t varying = all_or ^ all_and;
    for (int sh = 0; sh < 64; sh += 8) {
      if (((varying >> sh) & 0xffu) == 0) continue;  // every key has the same byte here
      size_t cnt8[257] = {0};
      for (uint64_t kx : keys) ++cnt8[((kx >> sh) & 0xffu) + 1];
      for (int b = 0; b < 256; ++b) cnt8[b + 1] += cnt8[b];
      for (uint64_t kx : keys) tmp[cnt8[(kx >> sh) & 0xffu]++] = kx;
      keys.swap(tmp);
    }
  } else {
    std::sort(keys.begin(), keys.end());
  }
}

// strip kernel: two tasks per wavefront, neighbours in the order of (column blocks, rows, columns) -- the wavefront
// steps through the larger of its two matrices; a task left over is paired with itself
void Chunk::pair_strips() {
  std::vector<int32_t> &sl = sx.stripe_lane;  // (scratch)
  std::vector<uint64_t> &keys = sx.strip_keys;
  keys.clear();
  chain_columns();
  for (size_t k = 0; k < cnt; ++k)
    if (cp[k].kind == kTaskStrip || cp[k].kind == kTaskChain) {
      // (blocks, rows, columns within the last block, index): 8 + 18 + 9 + 24 bits -- up to 256 blocks; a one-wavefront
      // task has one block and a chain at least two, so the two kinds stay apart
      const int bw = 64 * cp[k].nreg;
      keys.push_back(((uint64_t)(strip_blocks(cp[k].tlen, cp[k].nreg) - 1) << 51) | ((uint64_t)(uint32_t)cp[k].qlen << 33) |
                     ((uint64_t)(uint32_t)((cp[k].tlen - 1) % bw) << 24) | (uint64_t)k);
    }
  sort_strip_keys();
  sl.resize(keys.size());
  for (size_t q = 0; q < keys.size(); ++q) sl[q] = (int32_t)(keys[q] & 0xffffffu);
  for (size_t q = 0; q < sl.size();) {
    const int32_t x = sl[q];
    int32_t y = x;  // the next one, if it has as many column blocks and at most an eighth as many rows again (+ 64: the
                    // flag bound of cut_batch counts on it)
    if (q + 1 < sl.size() && cp[sl[q + 1]].kind == cp[x].kind &&
        strip_blocks(cp[sl[q + 1]].tlen, cp[x].nreg) == strip_blocks(cp[x].tlen, cp[x].nreg) &&
        cp[sl[q + 1]].qlen <= cp[x].qlen + cp[x].qlen / 8 + 64)
      y = sl[q + 1];
    q += y == x ? 1 : 2;
    const int32_t lo = std::min(x, y), hi = std::max(x, y);
    partner[lo] = hi;
    partner[hi] = lo;
    // (the rows the wavefront steps through: the traceback finds a block's records by it)
    cp[lo].ncol16 = cp[hi].ncol16 = std::max(cp[lo].qlen, cp[hi].qlen) | (lo == hi ? 1 << 30 : 0);  // (bit 30: no partner)
    if (cp[lo].kind == kTaskChain) {  // (the chain kernel finds a task's partner through its plan record)
      cp[lo].zdrop = hi;
      cp[hi].zdrop = lo;
    }
    if (lo != hi) c.paired += 2;
  }
}

// launch classes: (kernel, LDS bytes rounded to a power of two); the direction-flag layout inside this chunk's
// workspace region is fixed in the same pass (placed_dir_bytes: what cut_batch's bound is the maximum of)
bool Chunk::layout_and_classes() {
  cls.clear();
  size_t dir_acc = 0;
  for (size_t k = 0; k < cnt; ++k) {
    PlanTask &p = cp[k];
    // strips: one flag region per wavefront -- task A's words are the even, its partner's the odd ones of the same
    // records; placed with the task of the smaller index
    const bool strips = p.kind == kTaskStrip || p.kind == kTaskChain, second = strips && partner[k] < (int32_t)k;
    if (!second) {
      const bool alone = partner[k] < 0 || partner[k] == (int32_t)k;
      p.dir_off = (int64_t)dir_acc;
      if (strips && !alone) cp[partner[k]].dir_off = (int64_t)dir_acc + 4;
      dir_acc += placed_dir_bytes(p, alone ? p : cp[partner[k]], alone);
    }
  c.layouts |= 1u << dir_layout(p);
  const int width = general_width(p.ncol16, p.tlen);
  const int block = width > 1024 ? 1024 : width > 256 ? 256 : 64;  // 4 cells per thread and pass over the row
  LaunchClass lc{Family::General};
  size_t lds = 2048, need;
  if (p.kind == kTaskChain) {
    if (partner[k] < (int32_t)k) continue;  // (its partner's entry stands for both)
    lc = {Family::Chain, p.nreg};  // chained strips: one wavefront (workgroup) per block of 64 x nreg columns of a pair of tasks
    need = 16;
    lds = 1024;
  } else if (p.kind == kTaskStrip) {
    if (partner[k] < (int32_t)k) continue;  // placed together with its partner
    lc = {Family::Strip};  // strip kernel, one wavefront per pair of tasks
    need = strip_lds_bytes(std::max(p.qlen, cp[partner[k]].qlen), std::max(p.tlen, cp[partner[k]].tlen));
    lds = 1024;
    while (lds < need) lds *= 2;
  } else if (p.kind == kTaskPair) {
    if (partner[k] < (int32_t)k) continue;  // placed together with its partner
    lc = tracked[k] ? LaunchClass{Family::PairTrack, p.nreg} : mixedf[k] ? LaunchClass{Family::PairMixed, p.nreg}
                    : LaunchClass{Family::Pair, p.nreg, !pair_fits_whole(p.qlen, p.tlen, p.nreg)};
    need = mixedf[k] ? pair_mixed_lds_bytes(std::max(p.qlen, cp[partner[k]].qlen), std::max(p.tlen, cp[partner[k]].tlen), p.nreg)
                     : pair_lds_bytes(p.qlen, p.tlen, p.nreg);
    lds = 8192;
    while (lds < need) lds *= 2;
  } else if (p.kind == kTaskStripe) {
    lc = {Family::Stripe, p.nreg};  // stripe kernel, one wavefront (workgroup) per stripe
    need = stripe_lds_bytes(p.qlen, p.nreg);
    lds = 8192;
    while (lds < need) lds *= 2;
  } else if (p.kind == kTaskBStripe) {
    lc = {Family::BStripe, p.nreg};  // banded stripe kernel, one wavefront (workgroup) per stripe
    need = bstripe_lds_bytes(p.w, p.nreg);
    lds = 8192;
    while (lds < need) lds *= 2;
  } else if (p.nreg) {
    lc = {Family::Wave, p.nreg, !wave_fits_whole(p.qlen, p.tlen, p.nreg)};
    // one class for everything up to 6 KiB (>= 6 waves/SIMD either way), powers of two above
    need = wave_lds_bytes(p.qlen, p.tlen, p.nreg);
    lds = 6144;
    while (lds < need) lds *= 2;
  } else if (p.kind == kTaskGeneralHbm || p.kind == kTaskPlainHbm) {  // HBM-resident state: one class, slab = largest requirement
    lc = p.kind == kTaskPlainHbm ? LaunchClass{Family::GeneralPlainHbm, 0, false, 1024}
                                 : LaunchClass{Family::GeneralHbm, 0, false, width > 1024 ? 1024 : 256};
    need = general_lds_bytes(p.qlen, p.tlen);
    lds = (size_t)1 << 40;
  } else {
    lc = {p.kind == kTaskPlain ? Family::GeneralPlain : Family::General, 0, false, block};
    need = general_lds_bytes(p.qlen, p.tlen);
    while (lds < need) lds *= 2;
  }
  const bool hbm_cls = lc.hbm_state();
  if (!hbm_cls && need > (size_t)env.max_dyn_lds) {  // every kernel choice above checked its LDS need
    c.err = "internal: launch class needs more LDS than the device offers";
    return false;
  }
  if (!hbm_cls && lds > (size_t)env.max_dyn_lds) lds = env.max_dyn_lds;
  Cls *cl = nullptr;
  for (auto &x : cls)
    if (x.lc == lc && x.lds == lds) cl = &x;
  if (!cl) {
    cls.push_back({lc, lds, 0, {}});
    cl = &cls.back();
  }
  cl->need_max = std::max(cl->need_max, need);
  cl->est = std::max(cl->est, (double)(p.qlen + p.tlen) * (double)p.ncol16 / lc.rate());
  cl->idx.push_back((int32_t)k);
  if (p.kind == kTaskPair || p.kind == kTaskStrip) cl->idx.push_back(partner[k]);
}
  c.dir_bytes = dir_acc;
  if (dir_acc > (c.heavy ? cut.heavy_need : cut.region_need)) {
    c.err = "internal: direction-flag region overflow";
    return false;
  }
  return true;
}

// Small classes of one kernel (< 2048 tasks: occupancy is not what limits them, their longest task is) are
// merged into one launch with the largest LDS size among them: fewer launches queued one behind the other.
void Chunk::merge_classes() {
  for (size_t a = 0; a < cls.size(); ++a) {
    if (cls[a].idx.empty() || cls[a].idx.size() >= 2048) continue;
    for (size_t b = a + 1; b < cls.size(); ++b) {
      if (cls[b].lc != cls[a].lc || cls[b].idx.empty() || cls[b].idx.size() >= 2048) continue;
      cls[a].lds = std::max(cls[a].lds, cls[b].lds);
      cls[a].need_max = std::max(cls[a].need_max, cls[b].need_max);
      cls[a].est = std::max(cls[a].est, cls[b].est);
      cls[a].idx.insert(cls[a].idx.end(), cls[b].idx.begin(), cls[b].idx.end());
      cls[b].idx.clear();
    }
  }
  cls.erase(std::remove_if(cls.begin(), cls.end(), [](const Cls &x) { return x.idx.empty(); }), cls.end());
}

// inside a launch of few tasks the longest go first too (workgroups are dispatched in order: a long task that
// starts last is the tail of the launch); pair-kernel entries move as (task, partner) units
void Chunk::longest_first_in_class() {
  for (auto &x : cls) {
    // (a mixed class -- long and short tasks in one launch -- however large: the long chains start first)
    if ((x.idx.size() >= 8192 && !x.lc.mixed()) || x.idx.size() < 3) continue;
    auto work = [&](int32_t k) { return (int64_t)(cp[k].qlen + cp[k].tlen) * cp[k].ncol16; };
    int64_t wmin = work(x.idx[0]), wmax = wmin;
    for (int32_t k : x.idx) {
      const int64_t wk = work(k);
      wmin = std::min(wmin, wk);
      wmax = std::max(wmax, wk);
    }
    if (wmax < 2 * wmin) continue;  // tasks of one size: the order does not matter
    if (x.lc.two_per_entry()) {
      std::vector<std::pair<int32_t, int32_t>> pr(x.idx.size() / 2);
      for (size_t q = 0; q < pr.size(); ++q) pr[q] = {x.idx[2 * q], x.idx[2 * q + 1]};
      std::stable_sort(pr.begin(), pr.end(), [&](const std::pair<int32_t, int32_t> &a, const std::pair<int32_t, int32_t> &b) {
        return work(a.first) > work(b.first);
      });
      for (size_t q = 0; q < pr.size(); ++q) {
        x.idx[2 * q] = pr[q].first;
        x.idx[2 * q + 1] = pr[q].second;
      }
    } else {
      std::stable_sort(x.idx.begin(), x.idx.end(), [&](int32_t a, int32_t b) { return work(a) > work(b); });
    }
  }
}

// Stripe kernel: one entry per stripe, (stripe << 24) | task.  Workgroup i runs on XCD i mod 8 and workgroups
// are dispatched in index order.  The tasks are dealt to the eight residues (most stripes first, to the residue
// with the fewest so far): a task's stripes share an XCD (its L2 carries their edge words).  A task is a chain:
// stripe s starts 128 * nreg rows after stripe s - 1 and the last one ends qlen + tlen rows after the first
// began, and the launch ends with its longest chain.  Every residue lists its entries by the row at which they
// would have to start for all chains to END together -- s * 128 * nreg - (qlen + tlen) -- earliest first: the
// long tasks get their wavefront slots first (those of their later stripes sleep until their turn), the short
// ones fill in behind.  The key grows with s, so a stripe's left neighbour -- the only wavefront it ever waits
// for -- has a smaller index on the same XCD: resident or finished.
// (Entries with stripe index 255 do nothing: they keep the residues aligned where the lists differ in length.)
// (chained strips, extz2_strip.hip: an entry stands for a PAIR of tasks -- the one listed and its partner --, a
// "stripe" is a block of 512 columns of the wider of the two, 64 steps behind the block to its left, and the chain
// is as long as the rows of the longer plus 64 per block)
bool Chunk::deal_stripes(const Cls &x, size_t &cursor) {
  const bool chained = x.lc.fam == Family::Chain;
  const bool banded = x.lc.fam == Family::BStripe;  // (banded stripe kernel: stripes over the padded target, 2 * 128 * nreg rows apart)
  const int nreg = x.lc.nreg;
  const size_t first = cursor;
  const int nslot = chained ? 64 : banded ? 256 * nreg : 128 * nreg;  // rows between the starts of consecutive stripes
  auto stripes_of = [&](int32_t rel) {
    if (chained) return strip_blocks(std::max(cp[rel].tlen, cp[partner[rel]].tlen), nreg);
    return banded ? bstripe_geom(cp[rel].qlen, cp[rel].tlen, cp[rel].w, nreg).nst : (cp[rel].tlen + 128 * nreg - 1) / (128 * nreg);
  };
  auto chain_rows = [&](int32_t rel) {
    if (chained) return std::max(cp[rel].qlen, cp[partner[rel]].qlen) + 64 * stripes_of(rel);
    return cp[rel].qlen + cp[rel].tlen;
  };
  // (the start keys are taken in units of the rows between two stripes' starts: a counting sort per residue)
  int rq_max = 0, lane_sum[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int32_t rel : x.idx) rq_max = std::max(rq_max, chain_rows(rel) / nslot);
  const int nbucket = rq_max + 258;  // key of (task, s): s - (qlen + tlen) / nslot + rq_max, 0 <= s < 255
  std::vector<int32_t> &lane_of = sx.stripe_lane, &fill = sx.stripe_fill;
  lane_of.resize(x.idx.size());
  fill.assign((size_t)8 * nbucket + 1, 0);
  for (size_t j = 0; j < x.idx.size(); ++j) {
    const int32_t rel = x.idx[j];
    int to = 0;
    for (int q = 1; q < 8; ++q)
      if (lane_sum[q] < lane_sum[to]) to = q;
    const int nst = stripes_of(rel), key0 = rq_max - chain_rows(rel) / nslot;
    lane_of[j] = to;
    lane_sum[to] += nst;
    for (int sidx = 0; sidx < nst; ++sidx) ++fill[(size_t)to * nbucket + key0 + sidx + 1];
  }
  const int longest = *std::max_element(lane_sum, lane_sum + 8);
  if (cursor + (size_t)longest * 8 > c.order_cap) {
    c.err = "internal: launch-order segment overflow";
    return false;
  }
  for (size_t q = 0; q < (size_t)8 * nbucket; ++q) fill[q + 1] += fill[q];  // -> first position of (residue, key)
  {
    int base[8], acc = 0;  // positions are residue-relative
    for (int q = 0; q < 8; ++q) {
      base[q] = acc;
      acc += lane_sum[q];
    }
    const int32_t idle = (int32_t)((255u << 24) | (uint32_t)x.idx[0]);
    for (int pos = 0; pos < longest; ++pos)
      for (int q = 0; q < 8; ++q)
        if (pos >= lane_sum[q]) order[c.ob + first + (size_t)pos * 8 + q] = idle;
    for (size_t j = 0; j < x.idx.size(); ++j) {
      const int32_t rel = x.idx[j];
      const int to = lane_of[j], nst = stripes_of(rel), key0 = rq_max - chain_rows(rel) / nslot;
      for (int sidx = 0; sidx < nst; ++sidx) {
        const int pos = fill[(size_t)to * nbucket + key0 + sidx]++ - base[to];
        order[c.ob + first + (size_t)pos * 8 + to] = (int32_t)(((uint32_t)sidx << 24) | (uint32_t)rel);
      }
    }
    cursor = first + (size_t)longest * 8;
  }
  return true;
}

// longest launches first so the long tasks start early
void Chunk::launch_order() {
  std::sort(cls.begin(), cls.end(), [](const Cls &a, const Cls &b) { return a.est > b.est; });
  size_t cursor = 0;
  for (auto &x : cls) {
    const size_t lds_bytes = x.lc.hbm_state() ? ((x.need_max + 255) & ~(size_t)255) : std::min(x.lds, (x.need_max + 511) & ~(size_t)511);
    const size_t first = cursor;
    if (x.lc.per_stripe()) {
      if (!deal_stripes(x, cursor)) return;
    } else {
      std::copy(x.idx.begin(), x.idx.end(), order + c.ob + cursor);
      cursor += x.idx.size();
    }
    c.launches.push_back({x.lc, lds_bytes, first, cursor - first, x.est});
    if (x.lc.per_stripe())
      for (int32_t rel : x.idx) c.launches.back().rmax = std::max(c.launches.back().rmax, cp[rel].qlen + cp[rel].tlen);
  }
  c.nord = cursor;
  if (c.nord > c.order_cap) c.err = "internal: launch-order segment overflow";
}

}  // namespace

// Plans one chunk into plan[c.pb ...] and order[c.ob ...].
void plan_chunk(const PlanEnv &env, const BatchCut &cut, ChunkPlan &c, PlanTask *plan, int32_t *order, PlanScratch &sx) {
  const auto tp0 = std::chrono::steady_clock::now();
  auto tp1 = tp0, tp2 = tp0, tp3 = tp0;
  Chunk ch{env, cut, c, plan + c.pb, order, sx};
  ch.strips_or_not();
  ch.choose_kinds();
  tp1 = std::chrono::steady_clock::now();
  c.cnt = ch.cnt;
  c.nord = 0;
  c.launches.clear();
  c.layouts = 0;
  c.paired = 0;
  c.dir_bytes = 0;
  if (ch.cnt == 0) return;
  if (ch.n_stripe_tasks) ch.stripe_width();
  ch.mixed_or_not();
  ch.partner.assign(ch.cnt, -1);
  ch.tracked.assign(ch.cnt, 0);
  for (size_t k = 0; k < ch.cnt; ++k)
    if (ch.cp[k].kind == kTaskTrack) {
      ch.cp[k].kind = kTaskPair;
      ch.partner[k] = (int32_t)k;
      ch.tracked[k] = 1;
    }
  if (!env.cfg->no_pair && !env.force_general) {
    ch.pair_exact();
    if (ch.use_mixed) ch.pair_mixed();
    ch.pair_self();
  }
  ch.pair_strips();
  tp2 = std::chrono::steady_clock::now();
  if (!ch.layout_and_classes()) return;
  ch.merge_classes();
  ch.longest_first_in_class();
  tp3 = std::chrono::steady_clock::now();
  ch.launch_order();
  if (env.cfg->debug_plan != 0 && (c.heavy || env.cfg->debug_plan >= 2)) {
    auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    fprintf(stderr, "[plan_chunk %s %zu tasks: tasks %.2f ms, pairing %.2f ms, classes %.2f ms, order %.2f ms]\n", c.heavy ? "heavy" : "ordinary", c.cnt, ms(tp0, tp1), ms(tp1, tp2), ms(tp2, tp3), ms(tp3, std::chrono::steady_clock::now()));
  }
}

}  // namespace sdf
