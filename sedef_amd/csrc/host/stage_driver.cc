// The driver of `align generate`: the schedule, the super-batches and their lanes, several buckets in one process, resident
// chromosomes (restates reference src/align_main.cc:200-337).
#include <cmath>
#include <cstdlib>
#include <fstream>
#include <future>
#include <set>

#include "../../../include/sedef_hip.h"
#include <dirent.h>
#include <sys/stat.h>

#include "stage_internal.h"

namespace sdfh {

StageTotals g_totals;
void stage_totals_reset() { g_totals.records = g_totals.chars = g_totals.batches = g_totals.batches_resident = 0; }
void stage_totals(long long out[4]) {
  out[0] = g_totals.records, out[1] = g_totals.chars, out[2] = g_totals.batches, out[3] = g_totals.batches_resident;
}

bool resident_range(int64_t base, int64_t start, int64_t seq_len, int64_t s, int64_t len, bool rc, int64_t *off) {
  if (s < 0 || len < 0 || seq_len < 0 || s > seq_len || len > seq_len - s) return false;
  *off = rc ? base + start + seq_len - s - len : base + start + s;
  return true;
}

static int stage_super_batch(int total, int nlanes, int super_batch) {
  if (nlanes > 1) super_batch = std::max(1024, std::min(super_batch, (total + 2 * nlanes - 1) / (2 * nlanes)));
  if (stage_settings().super_batch > 0) super_batch = stage_settings().super_batch;
  return super_batch;
}

// Column `col` (from 0) of a tab-separated line that ends at a line end or a NUL: [first, second), empty where the line has
// fewer columns
static std::pair<const char *, const char *> bed_column(const char *line, int col) {
  const char *c = line, *e = c;
  for (;; c = e + 1, --col) {
    for (e = c; *e && *e != '\t' && *e != '\n';) ++e;
    if (col == 0 || *e != '\t') return {col == 0 ? c : e, e};
  }
}

StageHint stage_hint(const std::string &bed_path, int super_batch) {
  StageHint h;
  std::vector<int64_t> bytes;
  if (FILE *f = fopen(bed_path.c_str(), "rb")) {
    // columns 2, 3 and 5, 6 of a line: the two intervals (src/hit.cc: Hit::from_bed); anything else is skipped
    std::vector<char> line(1 << 16);
    auto num = [&](int col) { return (int64_t)atoll(bed_column(line.data(), col).first); };
    while (fgets(line.data(), (int)line.size(), f))
      bytes.push_back(std::max<int64_t>(0, num(2) - num(1)) + std::max<int64_t>(0, num(5) - num(4)));
    fclose(f);
  }
  h.pairs = (int)bytes.size();
  h.lanes = stage_lane_count(h.pairs, &h.devices);
  h.super_batch = stage_super_batch(h.pairs, h.lanes, super_batch);
  // the largest super-batch holds at most the `super_batch` largest pairs (and at most 1 GiB + one pair)
  const size_t k = std::min<size_t>(bytes.size(), (size_t)h.super_batch);
  std::partial_sort(bytes.begin(), bytes.begin() + (long)k, bytes.end(), std::greater<int64_t>());
  int64_t sum = 0;
  for (size_t i = 0; i < k && sum < ((int64_t)1 << 30); i++) sum += bytes[i];
  h.max_batch_bytes = (size_t)sum;
  return h;
}

int stage_lane_count(int total, std::vector<int> *devices) {
  // A second context costs 50-120 ms to set up, so small inputs stay on one lane; medium ones are cut into at least two
  // super-batches per lane.  (measured: 40,000 pairs 1.19 / 0.93 / 1.03 s with 2 / 3 / 4 lanes)
  int nlanes = total >= 12288 ? 3 : total >= 4096 ? 2 : 1;
  // SDF_DEVICES=0,1,...: the lanes after the first go round-robin over these devices (one node, several GPUs; the
  // first lane stays on the provider's own device, which should be the first of the list); at least one lane each
  const std::vector<int> &dv = stage_settings().devices;
  if (dv.size() > 1) nlanes = std::max<int>(nlanes, (int)std::min<size_t>(dv.size(), 8));
  if (stage_settings().lanes > 0) nlanes = std::max(1, std::min(8, stage_settings().lanes));
  if (devices) *devices = dv;
  return nlanes;
}

static std::vector<Hit> read_schedule(const std::string &bed_path, FILE *log) {  // src/align_main.cc:200-283, nbins=1
  std::ifstream fin(bed_path.c_str());
  if (!fin.is_open()) throw "BED file " + bed_path + " does not exist";
  // (the lines are parsed on the host threads: 40,000 lines take 26 ms on one)
  std::vector<std::string> text;
  std::string s;
  while (std::getline(fin, s)) text.push_back(std::move(s));
  std::vector<Hit> hits(text.size());
  parallel_for((int)text.size(), [&](int k) { hits[(size_t)k] = Hit::from_bed(text[(size_t)k]); });
  fprintf(log, "Read %d alignments in %s\n", (int)hits.size(), bed_path.c_str());
  fprintf(log, "Read total %d alignments\n", (int)hits.size());
  int max_complexity = 0;
  auto cx = [](const Hit &h) {
    return (int)std::sqrt(double(h.query_end - h.query_start) * double(h.ref_end - h.ref_start));
  };
  for (auto &h : hits) max_complexity = std::max(max_complexity, cx(h));
  // (a stable counting sort by bin, the records moved, not copied: a Hit owns two shared sequences and three strings)
  std::vector<int> bin(hits.size());
  std::vector<size_t> start(max_complexity / 1000 + 2, 0);
  for (size_t k = 0; k < hits.size(); k++) {
    bin[k] = cx(hits[k]) / 1000;
    start[(size_t)bin[k] + 1]++;
  }
  for (size_t b = 1; b < start.size(); b++) start[b] += start[b - 1];
  std::vector<Hit> order(hits.size());
  for (size_t k = 0; k < hits.size(); k++) order[start[(size_t)bin[k]]++] = std::move(hits[k]);
  return order;
}

namespace {
struct Acc {  // wall seconds of the phases of one lane of the driver
  double dp_secs = 0, anchor_secs = 0, t_fetch = 0, t_adv = 0, t_longest = 0, t_sum = 0, t_collect = 0, t_out = 0;
  int rounds = 0;
  int batches = 0, fetched_device = 0;  // super-batches, and those whose sequences came back from the device pool (SDF_STAGE_FETCH_DEVICE)
  Acc &operator+=(const Acc &o) {
    dp_secs += o.dp_secs, anchor_secs += o.anchor_secs, t_fetch += o.t_fetch, t_adv += o.t_adv;
    t_longest += o.t_longest, t_sum += o.t_sum, t_collect += o.t_collect, t_out += o.t_out;
    rounds += o.rounds, batches += o.batches, fetched_device += o.fetched_device;
    return *this;
  }
};

// What the super-batches of one run of the stage share.
struct StageRun {
  const Clock::time_point t0 = Clock::now();
  const bool dbg = stage_settings().debug_timing;
  Params p;
  std::vector<Hit> schedule;
  std::unique_ptr<FastaReference> fr;
  std::mutex cleanup_mu;
  std::vector<std::thread> cleanup;  // (threads that free the items of finished super-batches)
  // SDF_DEBUG_TIMING: one line per phase of every super-batch, milliseconds since the stage clock started
  void mark(int base, const char *what) const {
    if (dbg) fprintf(stderr, "[stage %7.1f ms] batch@%d %s\n", since(t0) * 1e3, base, what);
  }
  void join_cleanup() {
    for (auto &t : cleanup)
      if (t.joinable()) t.join();
    cleanup.clear();
  }
  ~StageRun() { join_cleanup(); }  // (also on the way out with an exception)
};

// A lane of the driver: its provider, its clocks, and the sequence pool of its super-batches when the provider has none
// (kept from super-batch to super-batch).
struct Lane {
  DpProvider *dp = nullptr;
  std::unique_ptr<DpProvider> own;  // (a lane after the first: its clone of the first lane's provider)
  Acc acc;
  std::unique_ptr<char[]> own_pool;
  size_t own_pool_cap = 0;
};

struct Item {
  Hit h;
  SeqView fa, fb;  // in the super-batch's pool (the provider's pinned staging, or the lane's own memory)
  std::unique_ptr<PairJob> job;
  std::vector<DpRequest> pending;
};

// One super-batch from the sequences to its formatted output lines (one string per pair, schedule order), phase by phase:
// fetch(), seed_anchors(), dp_rounds(), format().
struct SuperBatch {
  StageRun &run;
  Lane &lane;
  const int base, n;
  DpProvider &dp = *lane.dp;
  Acc &a = lane.acc;
  std::vector<Item> items = std::vector<Item>((size_t)n);
  std::vector<size_t> slot;  // pair k's query at pool + slot[2k], its reference at pool + slot[2k + 1]
  bool provider_pool = false;
  // resident chromosomes: the pairs name ranges of the pool the lane's provider reads (q_base / r_base: the first pool byte
  // of each pair's two ranges, in pool order), the host's copies below serve the host's own reads only
  const bool genome = lane.dp->has_genome();
  std::vector<DpProvider::AnchorBatch> seeds;  // (live until the jobs have taken their copies: their first advance)
  std::vector<int64_t> q_base = std::vector<int64_t>((size_t)n, 0), r_base = q_base;  // resident: the pairs in the device pool
  bool resident = false;
  std::vector<char> advanced = std::vector<char>((size_t)n, 0);  // pairs whose first advance() has run (requests in `pending`)
  std::atomic<long long> pre_us{0};

  void fetch() {
    run.mark(base, "start");
    const auto tf = Clock::now();
    // src/align_main.cc:299-306.  The bases of the whole super-batch go into ONE pool -- the provider's pinned staging when it
    // has one: the anchors call uploads from there without another copy, and the DP rounds name ranges of it -- a slot per
    // sequence as long as the bytes its range spans in the file (line ends included: the bound known before the copy).
    std::vector<FastaReference::Span> span(2 * (size_t)n);
    bool located = genome;  // resident chromosomes: every pair's two ranges are in q_base / r_base
    auto locate_resident = [&](const Sequence &s, int start, int64_t &at) {
      int64_t chr = 0;
      located = located && dp.chromosome_base(s.name, &chr);
      at = chr + std::max(0, start);
    };
    for (int k = 0; k < n; k++) {
      Item &it = items[k];
      it.h = run.schedule[base + k];
      span[2 * k] = run.fr->locate(it.h.query->name, it.h.query_start, &it.h.query_end);
      span[2 * k + 1] = run.fr->locate(it.h.ref->name, it.h.ref_start, &it.h.ref_end);
      if (located) locate_resident(*it.h.query, it.h.query_start, q_base[k]), locate_resident(*it.h.ref, it.h.ref_start, r_base[k]);
    }
    char *pool = nullptr;
    size_t bytes = 0;
    std::vector<size_t> need(2 * (size_t)n);
    auto lay_out = [&] {  // a slot of need[i] bytes per sequence, in the pool
      slot.assign(2 * (size_t)n + 1, 0);
      for (size_t i = 0; i < 2 * (size_t)n; i++) slot[i + 1] = slot[i] + need[i];
      bytes = slot[2 * (size_t)n];
      pool = genome ? nullptr : dp.pool_host(bytes + 1);
      provider_pool = pool != nullptr;
      if (!pool) {
        if (lane.own_pool_cap < bytes + 1) {
          lane.own_pool_cap = bytes + 1 + bytes / 8;
          lane.own_pool.reset(new char[lane.own_pool_cap]);
        }
        pool = lane.own_pool.get();
      }
    };
    auto make_jobs = [&](bool extract) {  // the pairs' sequences in their slots (extract: cut out of the file now), and their jobs
      parallel_for(n, [&](int k) {
        Item &it = items[k];
        char *qa = pool + slot[2 * k], *ra = pool + slot[2 * k + 1];
        it.fa = SeqView(qa, extract ? FastaReference::extract(span[2 * k], qa) : need[2 * k]);
        it.fb = SeqView(ra, extract ? FastaReference::extract(span[2 * k + 1], ra) : need[2 * k + 1]);
        if (extract && it.h.ref->is_rc) rc_inplace(ra, it.fb.size());
        it.job.reset(new PairJob(it.fa, it.fb, it.h, run.p, !genome));
      });
    };
    ++a.batches;
    std::vector<int64_t> off(genome ? 2 * (size_t)n : 0);  // resident chromosomes: the 2n ranges, as the device calls take them
    std::vector<int32_t> len(off.size());
    for (size_t k = 0; k < off.size() / 2; k++) off[2 * k] = q_base[k], off[2 * k + 1] = r_base[k];
    bool fetched = false;
    if (genome && stage_settings().fetch_device) {
      // Resident chromosomes hold these bases already: ONE device call of 2n ranges -- the query forward, the reference
      // reverse-complemented on its way where the hit says so -- writes them into slots as long as the bases (locate() has
      // clamped the ends).  A call that fails is said in one line, and this super-batch cuts its sequences out of the file.
      std::vector<char> rc(2 * (size_t)n, 0);
      std::string why = located ? "" : "a pair on a chromosome that is not resident";
      for (int k = 0; k < n && located; k++) {
        const Hit &h = items[k].h;
        len[2 * k] = span[2 * k].bytes ? std::max(0, h.query_end - std::max(0, h.query_start)) : 0;
        len[2 * k + 1] = span[2 * k + 1].bytes ? std::max(0, h.ref_end - std::max(0, h.ref_start)) : 0;
        rc[2 * k + 1] = h.ref->is_rc;
        need[2 * k] = (size_t)len[2 * k], need[2 * k + 1] = (size_t)len[2 * k + 1];
      }
      if (located) {
        lay_out();
        fetched = dp.fetch_ranges(off.data(), len.data(), rc.data(), slot.data(), off.size(), pool, bytes, why);
      }
      if (fetched) ++a.fetched_device;
      else
        fprintf(stderr, "[sedef_amd] SDF_STAGE_FETCH_DEVICE=1: super-batch at pair %d cuts its sequences out of the FASTA file: %s\n",
                base, why.c_str());
    }
    if (!fetched) {
      for (size_t i = 0; i < 2 * (size_t)n; i++) need[i] = span[i].bytes;
      lay_out();
    }
    make_jobs(!fetched);
    ++g_totals.batches;
    if (genome) {
      // Nothing is uploaded: the pairs' ranges of the resident chromosomes, and ONE device call that says which pairs hold
      // nothing but ACGTNacgtn (PairJob's own scan of every character otherwise).
      if (!located) throw std::string("internal: a pair on a chromosome that is not resident");
      std::vector<char> plain(2 * (size_t)n);
      for (int k = 0; k < n; k++) len[2 * k] = (int32_t)items[k].fa.size(), len[2 * k + 1] = (int32_t)items[k].fb.size();
      dp.plain_ranges(off.data(), len.data(), off.size(), plain.data());
      for (int k = 0; k < n; k++) items[k].job->set_exact(plain[2 * k] && plain[2 * k + 1]);
      ++g_totals.batches_resident;
    }
    a.t_fetch += since(tf);
    if (!genome) dp.pool_ready(bytes);  // (the whole pool to the device, asynchronously)
    run.mark(base, "sequences fetched");
  }

  // The parts the seed anchors are found in: part i holds pairs [cut[i], cut[i + 1]) -- parts of about equal bytes, two from
  // 16 MB of sequences, four from 64 MB (SDF_ANCHOR_PARTS), only where the sequences lie in the PROVIDER's pool (a provider
  // that copies them replaces its pool with every call).
  std::vector<int> part_cuts() const {
    const size_t total = slot[2 * (size_t)n];
    const bool on_device = provider_pool || genome;  // (resident chromosomes: no call replaces the pool)
    int parts = 1;
    if (on_device && n >= 64 && total >= ((size_t)16 << 20)) parts = 2;  // (small super-batches: one call)
    if (on_device && n >= 256 && total >= ((size_t)64 << 20)) parts = 4;
    if (stage_settings().anchor_parts > 0 && on_device) parts = std::min(stage_settings().anchor_parts, std::max(n / 16, 1));
    std::vector<int> cut((size_t)parts + 1, n);
    cut[0] = 0;
    for (int i = 1, k = 0; i < parts; i++) {
      while (k < n && slot[2 * (size_t)k] < total / (size_t)parts * (size_t)i) ++k;
      cut[i] = k;
    }
    for (int i = 0; i < parts; i++)
      if (cut[i + 1] - cut[i] < 16) return {0, n};  // (a part of a few pairs: one call for everything)
    return cut;
  }

  // The first advance() of pairs [lo, hi) -- chaining up to the requests of their round-A stitch (src/chain.cc:203-258) --
  // on the anchors `sd` holds for them.
  void first_advance(int lo, int hi, const DpProvider::AnchorBatch &sd) {
    parallel_for(hi - lo, [&](int i) {
      const int k = lo + i;
      const auto tj = Clock::now();
      items[k].job->set_anchors(sd.data() + sd.off[i], (size_t)(sd.off[i + 1] - sd.off[i]));
      items[k].pending = items[k].job->advance(std::vector<Cigar>());
      advanced[k] = 1;
      pre_us += std::chrono::duration_cast<std::chrono::microseconds>(Clock::now() - tj).count();
    });
  }

  // Seed anchors on the device, when the provider offers it -- in parts (part_cuts): while the device finds the anchors of
  // part i + 1, the host threads chain part i, which is the longest host phase of a super-batch (20 of 85 ms in the
  // chr1-sized run).  Every part's anchors are appended behind those of the parts before it in the provider's staging
  // (anchors_more), which stay valid until their jobs have taken their copies.  Without anchors from the device the jobs
  // find theirs on the host, in their first advance.
  void seed_anchors() {
    std::vector<DpProvider::AnchorJob> aj(n);
    for (int k = 0; k < n; k++) {
      const Hit &h = items[k].h;
      aj[k] = {items[k].fa, items[k].fb, h.query->name == h.ref->name && h.query->is_rc == h.ref->is_rc,
               h.ref_start - h.query_start};
      if (genome) aj[k].q_off = q_base[k], aj[k].r_off = r_base[k], aj[k].r_rc = h.ref->is_rc;
    }
    const std::vector<int> cut = part_cuts();
    const int parts = (int)cut.size() - 1;
    seeds.resize(parts);
    auto part_jobs = [&](int i) { return std::vector<DpProvider::AnchorJob>(aj.begin() + cut[i], aj.begin() + cut[i + 1]); };
    auto take_bases = [&](int i) {
      for (int k = cut[i]; k < cut[i + 1] && !genome; k++) {
        q_base[k] = resident ? seeds[i].q_base[k - cut[i]] : 0;
        r_base[k] = resident ? seeds[i].r_base[k - cut[i]] : 0;
      }
    };
    const auto ta = Clock::now();
    if (dp.anchors(part_jobs(0), run.p.kmer, seeds[0])) {
      resident = seeds[0].resident;
      take_bases(0);
      if (parts == 1) {
        for (int k = 0; k < n; k++)
          items[k].job->set_anchors(seeds[0].data() + seeds[0].off[k], (size_t)(seeds[0].off[k + 1] - seeds[0].off[k]));
      } else {
        size_t keep = (size_t)seeds[0].off[cut[1]];  // anchors in the staging so far
        bool have = true;                            // part i's anchors are there
        for (int i = 0; i < parts; i++) {
          const bool more = i + 1 < parts;
          const std::vector<DpProvider::AnchorJob> next_jobs = more ? part_jobs(i + 1) : std::vector<DpProvider::AnchorJob>();
          // (the next part's anchors on a thread of its own: whatever it throws arrives with get(), and the future waits for
          // the thread also on the way out with an exception)
          std::future<bool> next;
          if (more)
            next = std::async(std::launch::async, [&] { return dp.anchors_more(next_jobs, run.p.kmer, keep, seeds[i + 1]); });
          if (i == 0) run.mark(base, "anchors of the first part done");
          // (a part without anchors from the device: its jobs find theirs on the host, in their first advance)
          if (have) first_advance(cut[i], cut[i + 1], seeds[i]);
          if (!more) break;
          bool ok_next = next.get();
          // (no room behind the anchors of the parts before, or a part the device does not cover: the ordinary call, now
          // that the earlier parts' jobs have taken their copies -- it starts the staging over)
          bool fresh = false;
          if (!ok_next) ok_next = fresh = dp.anchors(next_jobs, run.p.kmer, seeds[i + 1]);
          have = ok_next;
          if (!ok_next) resident = false;  // (its pairs have no place in the resident pool the requests could name)
          if (ok_next && seeds[i + 1].resident != resident) resident = false;  // (the parts disagree about where the
                                                                              // sequences are: the pointer form for everybody)
          if (ok_next && resident) take_bases(i + 1);
          if (ok_next) keep = (fresh ? 0 : keep) + (size_t)seeds[i + 1].off[cut[i + 2] - cut[i + 1]];
        }
        run.mark(base, "anchors done");
      }
      a.anchor_secs += since(ta);
    }
    run.mark(base, "anchors done, parts chained");
  }

  // Every unfinished job advances on the results of the previous round: pair k's are requests [first[k], first[k + 1]) of
  // `raw`, turned into Cigars on the pair's own thread (which later frees them).
  void advance_jobs(const DpProvider::Raw &raw, const std::vector<size_t> &first) {
    const auto tadv = Clock::now();
    std::atomic<long long> longest_us(0), sum_us(0);
    parallel_for(n, [&](int k) {
      Item &it = items[k];
      if (advanced[k]) {  // (its first advance ran next to a later part's anchors: the requests are waiting)
        advanced[k] = 0;
        return;
      }
      it.pending.clear();
      if (it.job->done()) return;
      const auto tj = Clock::now();
      std::vector<Cigar> mine(first[k + 1] - first[k]);
      for (size_t r = 0; r < mine.size(); r++) mine[r] = raw.cigar(first[k] + r);
      it.pending = it.job->advance(mine);
      const long long us = std::chrono::duration_cast<std::chrono::microseconds>(Clock::now() - tj).count();
      sum_us += us;
      long long cur = longest_us.load();
      while (us > cur && !longest_us.compare_exchange_weak(cur, us)) {
      }
    });
    a.t_adv += since(tadv);
    a.t_longest += longest_us.load() / 1e6;
    a.t_sum += (sum_us.load() + pre_us.exchange(0)) / 1e6;
  }

  // Rounds: every unfinished job advances; all their DP requests go to the provider as one batch.
  void dp_rounds() {
    DpProvider::Raw raw;
    std::vector<size_t> first((size_t)n + 1, 0);  // pair k's requests of the round: [first[k], first[k + 1])
    for (;;) {
      advance_jobs(raw, first);
      const auto tc = Clock::now();
      for (int k = 0; k < n; k++) first[k + 1] = first[k] + items[k].pending.size();
      // (requests are four words each; with the pairs' characters on the device they become offsets of that pool, on the
      // host threads: 708,600 of them in the first round of the chr1-sized run)
      std::vector<DpRequest> batch(resident ? 0 : first[n]);
      std::vector<DpProvider::ResidentReq> rbatch(resident ? first[n] : 0);
      std::atomic<bool> outside(false);
      parallel_for(n, [&](int k) {
        Item &it = items[k];
        size_t at = first[k];
        if (resident) {
          const char *qa = it.fa.data(), *ra = it.fb.data();
          const bool rc = genome && it.h.ref->is_rc;  // (the host's copy of the reference is reverse-complemented)
          for (const DpRequest &r : it.pending) {
            int64_t qo = 0, to = 0;
            if (!resident_range(q_base[k], 0, (int64_t)it.fa.size(), r.q - qa, r.qlen, false, &qo) ||
                !resident_range(r_base[k], 0, (int64_t)it.fb.size(), r.t - ra, r.tlen, rc, &to))
              outside.store(true);
            rbatch[at++] = {qo, to, r.qlen, r.tlen, rc ? SDF_TASK_T_RC : 0};
          }
        } else {
          for (const DpRequest &r : it.pending) batch[at++] = r;
        }
        it.pending.clear();
      });
      if (outside.load()) throw std::string("internal: a DP request outside its pair's sequences");
      a.t_collect += since(tc);
      if (first[n] == 0) break;
      a.rounds++;
      run.mark(base, "jobs advanced, requests collected");
      const auto td = Clock::now();
      if (!resident) dp.run(batch, run.p, raw);
      else if (!dp.run_resident(rbatch, run.p, raw)) throw std::string("internal: the provider lost its resident sequences");
      a.dp_secs += since(td);
      run.mark(base, "DP round done");
    }
  }

  // The output lines (src/align_main.cc:314-331), formatted on the host threads; returns the hits.  The items go to the
  // cleanup thread.
  int format(std::vector<std::string> &lines) {
    const auto tout = Clock::now();
    lines.assign(n, std::string());
    std::atomic<int> hits(0);
    parallel_for(n, [&](int k) {
      Item &it = items[k];
      const std::string tail = "\t" + it.h.to_bed(false) + "\n";
      for (auto &hh : it.job->hits()) {
        hh.query_start += it.h.query_start;
        hh.query_end += it.h.query_start;
        if (it.h.ref->is_rc) {
          std::swap(hh.ref_start, hh.ref_end);
          hh.ref_start = it.h.ref_end - hh.ref_start;
          hh.ref_end = it.h.ref_end - hh.ref_end;
          hh.ref->is_rc = true;
        } else {
          hh.ref_start += it.h.ref_start;
          hh.ref_end += it.h.ref_start;
        }
        hh.query->name = it.h.query->name;
        hh.ref->name = it.h.ref->name;
        hits++;
        lines[k] += hh.to_bed(false);
        lines[k] += tail;
      }
    });
    a.t_out += since(tout);
    run.mark(base, "output formatted");
    // (the pairs' jobs hold hundreds of megabytes in small pieces: freeing them took a lane 15-50 ms between two
    // super-batches -- a thread of its own does it while the lane fetches the next one's sequences)
    auto *gone = new std::vector<Item>(std::move(items));
    std::lock_guard<std::mutex> g(run.cleanup_mu);
    run.cleanup.emplace_back([gone] { delete gone; });
    return hits;
  }
};

// Pairs per super-batch: every round of a super-batch is one device batch call (planning, launches, one synchronisation), so
// few large super-batches beat many small ones; bounded by the sequence bytes held at once.
struct Batch {
  int first, n;   // pairs [first, first + n) of the schedule
  int64_t bytes;  // their sequence
};
std::vector<Batch> cut_super_batches(const std::vector<Hit> &schedule, int super_batch) {
  std::vector<Batch> batches;
  const int total = (int)schedule.size();
  for (int base = 0, n = 0; base < total; base += n) {
    int64_t bytes = 0;
    n = 0;
    while (base + n < total && n < super_batch && bytes < ((int64_t)1 << 30)) {
      const Hit &h = schedule[(size_t)(base + n)];
      bytes += (int64_t)(h.query_end - h.query_start) + (h.ref_end - h.ref_start);
      ++n;
    }
    batches.push_back({base, n, bytes});
  }
  return batches;
}

void zero_counters(DpProvider &d) {  // (a provider serves bucket after bucket of one process: the figures are this run's)
  d.tasks = d.cells = 0;
  d.t_pack = d.t_call = d.t_unpack = 0;
}
}  // namespace

GenerateStats generate_alignments(const std::string &ref_path, const std::string &bed_path, int kmer_size,
                                  const Params &p_in, DpProvider &dp0, FILE *out, FILE *log, int super_batch) {
  StageRun run;
  run.p = p_in;
  run.p.kmer = kmer_size;
  set_alignment_scoring(run.p);
  GenerateStats st;
  g_us_chain = 0;
  g_us_rest = 0;
  run.schedule = read_schedule(bed_path, log);
  run.mark(-1, "schedule read");
  run.fr.reset(new FastaReference(ref_path));
  run.mark(-1, "fasta index open");
  fprintf(log, "Using k-mer size %d\n", kmer_size);
  const int total = (int)run.schedule.size();

  // Lanes: super-batches are independent, so two or three of them are in flight, each on its own device context -- while
  // one waits for the device, the host threads work on the other.  A second context costs ~0.1 s to set up, so
  // small inputs stay on one lane; medium ones are cut into at least two super-batches per lane.
  std::vector<int> devices;
  int nlanes = stage_lane_count(total, &devices);
  super_batch = stage_super_batch(total, nlanes, super_batch);
  const std::vector<Batch> batches = cut_super_batches(run.schedule, super_batch);
  int64_t max_batch_bytes = 0;
  for (const Batch &b : batches) max_batch_bytes = std::max(max_batch_bytes, b.bytes);
  dp0.prepare((size_t)max_batch_bytes);
  zero_counters(dp0);

  // Output is written in schedule order whatever lane produced it: a finished super-batch keeps its lines until every earlier
  // one of the schedule has been written.  The first lane runs on the calling thread; every other one creates its own device
  // context (~0.1 s) on its own thread while the first one is already working; the super-batches are handed out as the lanes
  // ask for them, so a lane that starts late, or cannot get a context at all, just takes fewer.
  nlanes = std::min<int>(nlanes, (int)batches.size());
  std::vector<Lane> lanes((size_t)std::max(nlanes, 1));
  lanes[0].dp = &dp0;
  // (several lanes take the super-batches with the most sequence first: the schedule is sorted by size, its last super-batch
  // is the heaviest, and taken last it ran on alone while the other lanes had nothing left; one lane keeps schedule order)
  std::vector<size_t> turn(batches.size());
  for (size_t b = 0; b < turn.size(); b++) turn[b] = b;
  if (nlanes > 1)
    std::stable_sort(turn.begin(), turn.end(), [&](size_t a, size_t b) { return batches[a].bytes > batches[b].bytes; });
  struct Done {  // a finished super-batch's output, until every earlier one has been written
    std::vector<std::string> lines;
    int hits = 0;
    bool ready = false;
  };
  std::vector<Done> done(batches.size());
  std::mutex mu;
  size_t next_write = 0;
  std::atomic<size_t> next_batch(0);
  FirstError failure;
  run_lanes((int)lanes.size(), failure, [&](int l) {
    Lane &lane = lanes[(size_t)l];
    if (l > 0) {
      try {
        lane.own = dp0.clone(devices.empty() ? -1 : devices[(size_t)l % devices.size()]);
      } catch (...) {  // no room for another device context: one lane fewer
      }
      lane.dp = lane.own.get();
      run.mark(-2 - l, "lane's device context ready");
      if (!lane.dp) return;
      if (lane.dp->has_genome() != dp0.has_genome()) {  // (it could not read the resident chromosomes: one lane fewer)
        dp0.give_back(std::move(lane.own));
        lane.dp = nullptr;
        return;
      }
      zero_counters(*lane.dp);
      lane.dp->prepare((size_t)max_batch_bytes);
    }
    for (size_t ti = next_batch++; ti < batches.size() && !failure.failed(); ti = next_batch++) {
      const size_t bi = turn[ti];
      SuperBatch sb{run, lane, batches[bi].first, batches[bi].n};
      sb.fetch();
      sb.seed_anchors();
      sb.dp_rounds();
      const int hits = sb.format(done[bi].lines);
      std::lock_guard<std::mutex> g(mu);
      if (failure.failed()) return;
      done[bi].hits = hits;
      done[bi].ready = true;
      // (whoever completes the next one in line writes)
      for (; next_write < batches.size() && done[next_write].ready; ++next_write) {
        const int end = batches[next_write].first + batches[next_write].n;
        st.lines += batches[next_write].n;
        st.total_written += done[next_write].hits;
        for (const std::string &line : done[next_write].lines)
          if (!line.empty()) fwrite(line.data(), 1, line.size(), out);
        std::vector<std::string>().swap(done[next_write].lines);
        fprintf(log, "\r Processing %d out of %d (%.1f%%)", end, total, 100.0 * end / std::max(total, 1));
      }
    }
  });
  failure.rethrow();
  const double secs = since(run.t0);  // (the output is complete; what is left is giving memory back)
  run.join_cleanup();
  Acc a;
  for (const Lane &l : lanes) a += l.acc;
  st.rounds = a.rounds;
  double t_pack = 0, t_call = 0, t_unpack = 0;
  for (const Lane &l : lanes) {
    if (!l.dp) continue;
    st.dp_tasks += l.dp->tasks;
    st.dp_cells += l.dp->cells;
    t_pack += l.dp->t_pack;
    t_call += l.dp->t_call;
    t_unpack += l.dp->t_unpack;
  }
  fprintf(log, "\nFinished BED %s in %.2fs (%d lines, generated %d hits)\n", bed_path.c_str(), secs, st.lines,
          st.total_written);
  fprintf(log, "  [%d lane(s); host CPU: anchors+chaining %.2fs, stitching+refinement %.2fs (summed over threads); device "
               "anchors %.2fs; DP provider %.2fs in %d rounds, %lld tasks, %.3g cells]\n",
          nlanes, g_us_chain.load() / 1e6, g_us_rest.load() / 1e6, a.anchor_secs, a.dp_secs, st.rounds,
          (long long)st.dp_tasks, (double)st.dp_cells);
  fprintf(log, "  [driver (summed over lanes): sequence fetch %.2fs, job rounds on host threads %.2fs (longest single jobs "
               "%.2fs, all jobs %.2fs thread time), request collection %.2fs, output %.2fs; DP provider: request "
               "packing %.2fs, device call %.2fs, CIGAR unpacking %.2fs]\n",
          a.t_fetch, a.t_adv, a.t_longest, a.t_sum, a.t_collect, a.t_out, t_pack, t_call, t_unpack);
  if (stage_settings().fetch_device && dp0.has_genome())  // (the marker that the device fetch ran, and how often it did not)
    fprintf(log, "  [sequence fetch: %d of %d super-batches read their sequences back from the device pool (SDF_STAGE_FETCH_DEVICE=1)]\n",
            a.fetched_device, a.batches);
  // (the extra lanes' providers go back to the one they came from: the next bucket of this process takes them again, and the
  // first provider gives all their device contexts back side by side when it goes)
  for (Lane &l : lanes)
    if (l.own) dp0.give_back(std::move(l.own));
  return st;
}

// ---- several buckets, one process --------------------------------------------------------------------------------
std::vector<std::string> expand_buckets(const std::vector<std::string> &beds) {
  std::vector<std::string> out;
  for (const std::string &b : beds) {
    struct stat sb;
    if (stat(b.c_str(), &sb) == 0 && S_ISDIR(sb.st_mode)) {
      // the bucket files `sedef align bucket` wrote there (src/align_main.cc:178: "bucket_{:04d}"), not the outputs next to them
      std::vector<std::string> names;
      if (DIR *d = opendir(b.c_str())) {
        while (struct dirent *e = readdir(d)) {
          const std::string n = e->d_name;
          if (n.size() == 11 && n.compare(0, 7, "bucket_") == 0 && n.find_first_not_of("0123456789", 7) == std::string::npos)
            names.push_back(n);
        }
        closedir(d);
      }
      std::sort(names.begin(), names.end());
      for (auto &n : names) out.push_back(b + (b.empty() || b.back() == '/' ? "" : "/") + n);
    } else {
      out.push_back(b);
    }
  }
  return out;
}

StageHint stage_hint_many(const std::vector<std::string> &beds, int super_batch) {
  StageHint all;
  all.pairs = 0;
  for (const std::string &b : beds) {
    const StageHint h = stage_hint(b, super_batch);
    all.pairs += h.pairs;
    if (h.lanes > all.lanes) {
      all.lanes = h.lanes;
      all.devices = h.devices;
    }
    all.super_batch = std::max(all.super_batch, h.super_batch);
    all.max_batch_bytes = std::max(all.max_batch_bytes, h.max_batch_bytes);
  }
  // (one-lane buckets run SDF_BUCKET_LANES at a time, generate_many: a provider each)
  if (all.lanes <= 1 && beds.size() >= 2 && stage_settings().bucket_lanes > 1)
    all.lanes = (int)std::min<size_t>((size_t)stage_settings().bucket_lanes, beds.size());
  return all;
}

bool load_stage_genome(DpProvider &dp, const std::string &ref_path, const std::vector<std::string> &beds, int kmer,
                       size_t max_batch_bytes, FILE *log) {
  const StageSettings &st = stage_settings();
  if (!st.stage_resident) return false;
  std::string why;
  if (kmer > 15) why = "k-mer sizes above 15 find their seed anchors on the host";
  else if (!st.resident_dp) why = "SDF_RESIDENT_DP=0";
  else if (!st.gpu_anchors) why = "SDF_GPU_ANCHORS=0";
  else if (st.devices.size() > 1) why = "the lanes are on several devices";
  bool ok = false;
  if (why.empty()) {
    // the chromosomes the seed pairs name: columns 1 and 4 of every line (src/hit.cc: Hit::from_bed), in order of appearance
    std::vector<std::string> names;
    std::set<std::string> seen;
    for (const std::string &bed : beds) {
      std::ifstream fin(bed.c_str());
      std::string line;
      while (std::getline(fin, line))
        for (int col : {0, 3}) {
          const auto c = bed_column(line.c_str(), col);
          if (c.second > c.first && seen.insert(std::string(c.first, c.second)).second) names.emplace_back(c.first, c.second);
        }
    }
    const auto t0 = Clock::now();
    FastaReference fr(ref_path);
    ok = dp.load_genome(fr, names, max_batch_bytes, why);
    if (ok && st.debug_timing)
      fprintf(log, "[resident chromosomes: %zu records loaded and shared in %.1f ms]\n", names.size(), since(t0) * 1e3);
  }
  if (!ok) fprintf(log, "[sedef_amd] SDF_STAGE_RESIDENT=1 ignored, every bucket runs on uploaded super-batches: %s\n", why.c_str());
  return ok;
}

// One bucket of generate_many: its lines to `<bed><out_suffix>`, its log to `<log_dir>/<basename>.log` with a log directory,
// else to `log` -- with `buffer_log` (buckets in flight at once, whose progress lines would interleave on the shared log)
// through a buffer that reaches `log` in one piece when the bucket is over, also when it failed.  A file that cannot be
// opened throws before the bucket starts.
static GenerateStats run_bucket(const std::string &ref_path, const std::string &bed, int kmer_size, const Params &p,
                                DpProvider &dp, const std::string &out_suffix, const std::string &log_dir, FILE *log,
                                int super_batch, std::mutex &log_mu, bool buffer_log) {
  typedef std::unique_ptr<FILE, int (*)(FILE *)> File;
  const std::string out_path = bed + out_suffix;
  File out(fopen(out_path.c_str(), "w"), fclose), blog(nullptr, fclose);
  if (!out) throw std::string("Cannot open file ") + out_path + " for writing";
  if (!log_dir.empty()) {
    const size_t slash = bed.find_last_of('/');
    const std::string lp = log_dir + "/" + (slash == std::string::npos ? bed : bed.substr(slash + 1)) + ".log";
    blog.reset(fopen(lp.c_str(), "w"));
    if (!blog) throw std::string("Cannot open file ") + lp + " for writing";
  }
  struct MemLog {
    FILE *f, *to;
    std::mutex &mu;
    char *buf = nullptr;
    size_t len = 0;
    ~MemLog() {
      if (!f) return;
      fclose(f);
      std::lock_guard<std::mutex> g(mu);
      if (len) fwrite(buf, 1, len, to);
      free(buf);
    }
  } mem{nullptr, log, log_mu};
  if (!blog && buffer_log) mem.f = open_memstream(&mem.buf, &mem.len);
  FILE *blog_or_log = blog ? blog.get() : mem.f ? mem.f : log;
  const GenerateStats st = generate_alignments(ref_path, bed, kmer_size, p, dp, out.get(), blog_or_log, super_batch);
  out.reset();
  if (blog) {
    blog.reset();
    std::lock_guard<std::mutex> g(log_mu);
    fprintf(log, "Finished BED %s (%d lines, generated %d hits)\n", bed.c_str(), st.lines, st.total_written);
  }
  return st;
}

std::vector<GenerateStats> generate_many(const std::string &ref_path, const std::vector<std::string> &beds, int kmer_size,
                                         const Params &p, DpProvider &dp, const std::string &out_suffix,
                                         const std::string &log_dir, FILE *log, int super_batch) {
  // One bucket's phases use the host and the device in turn (sequence fetch, anchors, ~65 ms of chaining on all threads, DP
  // rounds, output): with several one-lane buckets to do, SDF_BUCKET_LANES of them (default 2) are in flight, each on a
  // provider -- a device context -- of its own, taking buckets as they go.  A bucket's output file and log are its own,
  // its lines are what a process of its own writes; the order of the "Finished" lines on the shared log is the order of
  // completion.  (Buckets large enough for several lanes of super-batches run one after the other: their lanes fill the gaps.)
  size_t conc = 1;
  if (beds.size() >= 2 && stage_settings().bucket_lanes > 1) {
    bool one_lane = true;
    for (const std::string &bed : beds) one_lane = one_lane && stage_hint(bed, super_batch).lanes <= 1;
    if (one_lane) conc = std::min<size_t>((size_t)stage_settings().bucket_lanes, beds.size());
  }
  std::vector<GenerateStats> all(beds.size());
  std::mutex log_mu;
  if (conc <= 1) {
    for (size_t bi = 0; bi < beds.size(); bi++)
      all[bi] = run_bucket(ref_path, beds[bi], kmer_size, p, dp, out_suffix, log_dir, log, super_batch, log_mu, false);
    return all;
  }
  Params pk = p;
  pk.kmer = kmer_size;
  set_alignment_scoring(pk);  // (before the threads: generate_alignments finds it in place)
  std::vector<std::unique_ptr<DpProvider>> extra(conc);
  std::atomic<size_t> next(0);
  FirstError failure;
  run_lanes((int)conc, failure, [&](int l) {
    DpProvider *d = &dp;
    if (l > 0) {
      try {
        extra[(size_t)l] = dp.clone(-1);
      } catch (...) {  // (no room for another device context: one bucket lane fewer)
      }
      d = extra[(size_t)l].get();
      if (!d) return;
    }
    for (size_t bi = next++; bi < beds.size() && !failure.failed(); bi = next++)
      all[bi] = run_bucket(ref_path, beds[bi], kmer_size, p, *d, out_suffix, log_dir, log, super_batch, log_mu, true);
  });
  for (auto &e : extra)
    if (e) dp.give_back(std::move(e));
  failure.rethrow();
  return all;
}

}  // namespace sdfh
