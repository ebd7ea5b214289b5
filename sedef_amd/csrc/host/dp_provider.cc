// DP providers: align_helper (src/align.cc:39-68) for a batch of requests -- on a HIP device (GpuProvider), or through the
// test hook (TestProvider).
#include <cstdlib>
#include <cstring>

#include "../../../include/sedef_hip.h"
#include "stage_internal.h"

namespace sdfh {

namespace {

struct TaskRef {
  size_t req;
  size_t q_off, t_off;
  int qlen, tlen;
};

// chunking of one request into DP tasks (src/align.cc:46-57): both sequences advance by the same SP -- f(sp, ql, tl) for
// every chunk, in order; returns their number, which is chunk_count's
size_t chunk_step(const Params &p) { return (size_t)p.max_ksw_seq_len; }
size_t chunk_count(int qlen, int tlen, size_t step) { return ((size_t)std::min(qlen, tlen) + step - 1) / step; }
template <class F>
size_t for_each_chunk(int qlen, int tlen, size_t step, F f) {
  const size_t lim = (size_t)std::min(qlen, tlen);
  size_t n = 0;
  for (size_t sp = 0; sp < lim; sp += step, n++)
    f(sp, (int)std::min<size_t>(step, (size_t)qlen - sp), (int)std::min<size_t>(step, (size_t)tlen - sp));
  return n;
}
// (a reversed target is read from the END of its range: chunk sp holds its bases [sp, sp + tl))
int64_t chunk_target(int64_t t_off, int tlen, size_t sp, int tl, bool rc) {
  return rc ? t_off + tlen - (int64_t)sp - tl : t_off + (int64_t)sp;
}

// A round of the stage holds hundreds of thousands of requests (708,600 in the chr1-sized run): offsets and task counts in one
// serial pass, the copies and the task records on the host threads, the pool left unfilled where nothing is copied.
struct TaskPool {
  std::unique_ptr<uint8_t[]> bytes;
  size_t size = 0;
  const uint8_t *data() const { return bytes.get(); }
};
struct AlignCodes {  // align_dna (src/common.h:60-70,91): ACGT of either case 0..3, anything else the wildcard 4
  uint8_t of[256];
  AlignCodes() {
    for (int c = 0; c < 256; c++) {  // (the table is indexed with c & 127, like the host's align_dna)
      const int u = (c & 127) & ~0x20;
      of[c] = u == 'A' ? 0 : u == 'C' ? 1 : u == 'G' ? 2 : u == 'T' ? 3 : 4;
    }
  }
};
const AlignCodes kCodes;
// (`first`: per request (+1), its first task, as Raw::first_task)
void expand(const std::vector<DpRequest> &reqs, const Params &p, std::vector<TaskRef> &tasks, TaskPool &pool,
            std::vector<size_t> &first) {
  const size_t n = reqs.size(), step = chunk_step(p);
  std::vector<size_t> off(n + 1, 0);
  first.assign(n + 1, 0);
  for (size_t k = 0; k < n; k++) {
    const DpRequest &r = reqs[k];
    off[k + 1] = off[k] + (size_t)r.qlen + (size_t)r.tlen;
    first[k + 1] = first[k] + chunk_count(r.qlen, r.tlen, step);
  }
  pool.size = off[n];
  pool.bytes.reset(new uint8_t[std::max<size_t>(off[n], 1)]);
  tasks.resize(first[n]);
  parallel_blocks(n, 4096, [&](size_t lo, size_t hi) {
    for (size_t k = lo; k < hi; k++) {
      const DpRequest &r = reqs[k];
      const size_t qo = off[k], to = qo + (size_t)r.qlen;
      uint8_t *dq = pool.bytes.get() + qo, *dt = pool.bytes.get() + to;
      for (int i = 0; i < r.qlen; i++) dq[i] = kCodes.of[(unsigned char)r.q[i]];
      for (int i = 0; i < r.tlen; i++) dt[i] = kCodes.of[(unsigned char)r.t[i]];
      size_t at = first[k];
      for_each_chunk(r.qlen, r.tlen, step, [&](size_t sp, int ql, int tl) { tasks[at++] = {k, qo + sp, to + sp, ql, tl}; });
    }
  });
}

inline void append_ops(Cigar &c, const uint32_t *w, int64_t n) {
  for (int64_t i = 0; i < n; i++) {
    const int idx = w[i] & 0xf, len = (int)(w[i] >> 4);
    if (idx < 3) c.push_back({"MDI"[idx], len});  // ksw I (query) -> 'D', ksw D (target) -> 'I'
  }
}

void fill_mat(const Params &p, int8_t mat[25]) {  // src/align.cc:41-44
  const int8_t a = (int8_t)p.match, b = p.mismatch < 0 ? (int8_t)p.mismatch : (int8_t)(-p.mismatch);
  const int8_t m[25] = {a, b, b, b, 0, b, a, b, b, 0, b, b, a, b, 0, b, b, b, a, 0, 0, 0, 0, 0, 0};
  memcpy(mat, m, 25);
}

class GpuProvider : public DpProvider {
 public:
  // (`spares`: that many more providers, started before this one's own context so that all of them are set up side by side)
  // `max_batch_bytes` (0: unknown, prepare() will tell): the buffers are sized here, with the context.
  // `lanes`: the providers that share the device's memory with this one (itself included): the workspace budget is per process.
  explicit GpuProvider(int device, int spares = 0, const std::vector<int> &devices = std::vector<int>(),
                       size_t max_batch_bytes = 0, int lanes = 0)
      : device_(device), ws_(stage_workspace(lanes > 0 ? lanes : spares + 1)), lanes_(lanes > 0 ? lanes : spares + 1) {
    if (spares > 0) start_spares(spares, devices, max_batch_bytes);
    ctx_ = sdf_create(device, ws_);
    if (!ctx_) {
      join_spares();
      throw std::string("GPU DP backend unavailable: ") + sdf_last_error(nullptr);
    }
    if (max_batch_bytes) {
      prepared_ = true;
      reserve(max_batch_bytes);
    }
  }
  ~GpuProvider() override {
    ready();
    join_spares();
    {  // (the spare lanes' device contexts side by side: a context takes 30-40 ms to give back)
      std::vector<std::thread> gone;
      for (Spare &s : spares_)
        if (s.p) gone.emplace_back([&s] { s.p.reset(); });
      for (auto &t : gone) t.join();
    }
    spares_.clear();
    sdf_destroy(ctx_);
  }
  // Direction-flag workspace of a stage lane: 16 GiB per process (round 6: the far-gap round of a chr1-sized bucket -- 10,813
  // tasks whose flag bound is 15 GB -- then runs as ONE chunk, one 7 ms chain instead of two: its DP 14.6 -> 10.2 ms,
  // profiles/r06_stage_dp2.txt; 8 GiB until then), shared out over its lanes (at least 2 GiB each), unless
  // SDF_STAGE_WS_GIB gives the figure per lane (the library's default is 64).  A round of the stage that needs more runs in
  // chunks; in exchange a lane allocates its workspace ONCE, where it is set up.  A process that starts right after another
  // one released tens of gigabytes sometimes waits SECONDS for a large hipMalloc (profiles/alloc_probe.py: 24 and 64 GiB
  // 0.3 ms or 1.8-4.0 s, 8 GiB 0.3 ms in every sample; inside a stage run: a 23 GiB request 0.4 or 580 ms) -- and a run of
  // `sedef align` is one such process per bucket, one after the other.  (Measured at the end of round 6 for 16 GiB as well:
  // the CLI asks for 8 when it is given ONE bucket, sedef_main.cc, profiles/r06_proc_probe.txt.)
  static size_t stage_workspace(int lanes) {
    const double asked = stage_settings().stage_ws_gib;
    const double gib = asked > 0 ? asked : std::max(2.0, 16.0 / std::max(lanes, 1));
    return (size_t)(gib * 1073741824.0);
  }
  // Spare providers for the other lanes, each created on a thread of its own (make_gpu_providers)
  void start_spares(int n, const std::vector<int> &devices, size_t max_batch_bytes) {
    spares_.resize((size_t)n);
    for (int i = 0; i < n; i++) {
      const int dev = spares_[(size_t)i].device = devices.empty() ? device_ : devices[(size_t)(i + 1) % devices.size()];
      spares_[(size_t)i].starting = std::thread([this, i, n, dev, max_batch_bytes] {
        try {
          spares_[(size_t)i].p.reset(new GpuProvider(dev, 0, std::vector<int>(), max_batch_bytes, n + 1));
        } catch (...) {  // (no room for another context: clone() will try again, the lane does without)
        }
      });
    }
  }
  std::unique_ptr<DpProvider> clone(int device = -1) override {
    const int want = device < 0 ? device_ : device;
    {
      std::lock_guard<std::mutex> g(spare_mu_);
      for (Spare &s : spares_) {
        if (s.device != want || s.taken) continue;
        s.taken = true;
        if (s.starting.joinable()) s.starting.join();
        if (s.p) return std::unique_ptr<DpProvider>(s.p.release());
      }
    }
    // (a pool is shared where the contexts are set up, include/sedef_hip.h: a context made now could not read the genome)
    if (genome_) throw std::string("no spare device context reads the resident chromosomes");
    return std::unique_ptr<DpProvider>(new GpuProvider(want, 0, std::vector<int>(), 0, 3));
  }
  void give_back(std::unique_ptr<DpProvider> p) override {
    GpuProvider *g = dynamic_cast<GpuProvider *>(p.get());
    if (!g) return;
    std::lock_guard<std::mutex> lk(spare_mu_);
    p.release();
    for (Spare &s : spares_)
      if (s.taken && !s.p && s.device == g->device_) {
        s.p.reset(g);
        s.taken = false;
        return;
      }
    spares_.emplace_back();  // (made by clone() beyond the spares the provider started with: one more place)
    spares_.back().p.reset(g);
    spares_.back().device = g->device_;
  }
  // Buffers sized once per lane (include/sedef_hip.h: sdf_reserve), on a thread of its own.  The bounds follow the stage's
  // rounds as measured: a task per ~250 bytes of a super-batch's sequences at most (chr1-sized run: 708,600 tasks of
  // 182 MB), a tenth of the bytes as bases of DP tasks.
  // (a provider that was not told the size when it was set up -- the C ABI's generate entry point -- sizes its buffers on a
  // thread of its own while the driver fetches sequences; pinning next to the first anchors upload slows that one down,
  // include/sedef_hip.h: sdf_reserve)
  void prepare(size_t max_batch_bytes) override {
    if (prepared_) return;
    prepared_ = true;
    reserve_thread_ = std::thread([this, max_batch_bytes] { reserve(max_batch_bytes); });
  }
  void reserve(size_t max_batch_bytes) {
    const size_t tasks = max_batch_bytes / 250 + 65536, bases = max_batch_bytes / 6 + (1u << 20);
    const auto t0 = Clock::now();
    const int rc = sdf_reserve(ctx_, tasks, bases, ws_, SDF_RESERVE_BRIEF | SDF_RESERVE_ANCHORS | (lanes_ > 1 ? SDF_RESERVE_FEW_STREAMS : 0u));
    // (the super-batch's characters are written straight into pinned memory and cross PCIe as one DMA: sized here, once)
    // (a sequence's slot is as long as its range in the FILE -- a line end per 50-80 bases --, and a pair's end may move to the
    // chromosome's: a sixteenth more than the bases, so that the stage never pins a second time)
    if (stage_settings().gpu_anchors) (void)sdf_pool_host(ctx_, max_batch_bytes + max_batch_bytes / 16 + (1u << 20));
    if (stage_settings().debug_timing)
      fprintf(stderr, "[sdf_reserve tasks %zu bases %zu: rc %d, %.1f ms]\n", tasks, bases, rc, since(t0) * 1e3);
  }
  void ready() {
    if (reserve_thread_.joinable()) reserve_thread_.join();
  }
  void run(const std::vector<DpRequest> &reqs, const Params &p, Raw &raw) override {
    raw.first_task.assign(reqs.size() + 1, 0);
    raw.recs = nullptr;
    raw.words = nullptr;
    if (reqs.empty()) return;
    std::vector<TaskRef> tr;
    TaskPool pool;
    const auto tp0 = Clock::now();
    expand(reqs, p, tr, pool, raw.first_task);
    if (tr.empty()) return;
    const size_t nt = tr.size();
    std::unique_ptr<sdf_task[]> tasks(new sdf_task[nt]);
    parallel_blocks(nt, kTaskBlock, [&](size_t lo, size_t hi) {
      for (size_t k = lo; k < hi; k++) tasks[k] = make_task((int64_t)tr[k].q_off, (int64_t)tr[k].t_off, tr[k].qlen, tr[k].tlen);
    });
    call_batch(tasks.get(), nt, &pool, p, raw, tp0);
  }

  // The same round on ranges of the character pool the last anchors() call left on the device: nothing is cut out, coded,
  // packed or uploaded here (include/sedef_hip.h: sdf_extz2_batch_pairs) -- a request becomes its 60 kb chunks
  // (for_each_chunk) and that is all the host does per task.
  bool run_resident(const std::vector<ResidentReq> &reqs, const Params &p, Raw &raw) override {
    if (!resident_) return false;
    const size_t n = reqs.size(), step = chunk_step(p);
    raw.first_task.assign(n + 1, 0);
    raw.recs = nullptr;
    raw.words = nullptr;
    if (reqs.empty()) return true;
    const auto tp0 = Clock::now();
    std::vector<size_t> bfirst((n + kTaskBlock - 1) / kTaskBlock + 1, 0);
    parallel_blocks(n, kTaskBlock, [&](size_t lo, size_t hi) {
      size_t c = 0;
      for (size_t k = lo; k < hi; k++) c += chunk_count(reqs[k].qlen, reqs[k].tlen, step);
      bfirst[lo / kTaskBlock + 1] = c;
    });
    for (size_t b = 0; b + 1 < bfirst.size(); b++) bfirst[b + 1] += bfirst[b];
    const size_t nt = bfirst.back();
    raw.first_task[n] = nt;
    if (nt == 0) {
      std::fill(raw.first_task.begin(), raw.first_task.end(), 0);
      return true;
    }
    std::unique_ptr<sdf_task[]> tasks(new sdf_task[nt]);
    parallel_blocks(n, kTaskBlock, [&](size_t lo, size_t hi) {
      size_t at = bfirst[lo / kTaskBlock];
      for (size_t k = lo; k < hi; k++) {
        const ResidentReq &r = reqs[k];
        raw.first_task[k] = at;
        for_each_chunk(r.qlen, r.tlen, step, [&](size_t sp, int ql, int tl) {
          tasks[at++] = make_task(r.q_off + (int64_t)sp, chunk_target(r.t_off, r.tlen, sp, tl, r.flag & SDF_TASK_T_RC), ql, tl, r.flag);
        });
      }
    });
    call_batch(tasks.get(), nt, nullptr, p, raw, tp0);
    return true;
  }

 private:
  static constexpr size_t kTaskBlock = 16384;  // tasks (or requests) a host thread takes at a time
  static sdf_task make_task(int64_t q_off, int64_t t_off, int qlen, int tlen, int flag = 0) {
    sdf_task t;
    memset(&t, 0, sizeof(t));
    t.q_off = q_off;
    t.t_off = t_off;
    t.qlen = qlen;
    t.tlen = tlen;
    t.w = -1;      // src/align.cc:86
    t.zdrop = -1;  // src/align.cc:54
    t.flag = flag;
    return t;
  }
  // one device batch call and its results as Raw: `pool` holds the tasks' codes (offsets are bytes of it), or is NULL when the
  // offsets are ranges of the resident character pool
  void call_batch(const sdf_task *tasks, size_t nt, const TaskPool *pool, const Params &p, Raw &raw, Clock::time_point tp0) {
    std::atomic<size_t> cap_sum(0);
    std::atomic<int64_t> cells_sum(0);
    parallel_blocks(nt, kTaskBlock, [&](size_t lo, size_t hi) {
      size_t cap_b = 0;
      int64_t cells_b = 0;
      for (size_t k = lo; k < hi; k++) {
        cap_b += (size_t)tasks[k].qlen + tasks[k].tlen + 2;
        cells_b += (int64_t)tasks[k].qlen * tasks[k].tlen;
      }
      cap_sum += cap_b, cells_sum += cells_b;
    });
    const size_t cap = cap_sum;
    cells += cells_sum;
    this->tasks += (int64_t)nt;
    sdf_scoring sc;
    memset(&sc, 0, sizeof(sc));
    sc.m = 5;
    fill_mat(p, sc.mat);
    sc.gapo = (int8_t)(-p.gap_open);
    sc.gape = (int8_t)(-p.gap_extend);
    static_assert(sizeof(Raw::Rec) == sizeof(sdf_result_brief), "layouts must agree");
    size_t used = 0;
    ready();
    const auto tp1 = Clock::now();
    int rc;
    if (pool) {
      // (plain arrays, not std::vectors: the CIGAR capacity is the worst case, hundreds of megabytes that would be
      // zero-filled and paged in although the call writes only the words it reports in `used`)
      raw.own_recs.reset(new Raw::Rec[nt]);
      raw.own_words.reset(new uint32_t[cap]);
      rc = sdf_extz2_batch_brief(ctx_, &sc, tasks, nt, pool->data(), pool->size, (sdf_result_brief *)raw.own_recs.get(),
                                 raw.own_words.get(), cap, &used);
      raw.recs = raw.own_recs.get();
      raw.words = raw.own_words.get();
    } else {  // (read where the device's copies land: nothing is copied out of the pinned staging)
      const sdf_result_brief *res = nullptr;
      rc = sdf_extz2_batch_pairs_view(ctx_, &sc, tasks, nt, &res, &raw.words, &used);
      raw.recs = (const Raw::Rec *)res;
    }
    if (rc != SDF_OK) throw std::string("DP batch failed: ") + sdf_last_error(ctx_);
    const auto tp2 = Clock::now();
    t_pack += std::chrono::duration<double>(tp1 - tp0).count();
    t_call += std::chrono::duration<double>(tp2 - tp1).count();
  }

 public:
  char *pool_host(size_t bytes) override {
    if (!stage_settings().gpu_anchors || genome_) return nullptr;
    ready();
    uploaded_ = 0;
    pool_ = sdf_pool_host(ctx_, bytes + 64);
    pool_cap_ = pool_ ? bytes + 64 : 0;
    return pool_;
  }

  void pool_ready(size_t bytes) override {
    uploaded_ = 0;
    if (!pool_ || !stage_settings().gpu_anchors || bytes > pool_cap_ || genome_) return;
    if (sdf_pool_upload(ctx_, pool_, bytes) == SDF_OK) uploaded_ = bytes, g_totals.chars += (long long)bytes;
  }

  // what the device kernels do not cover goes to the host's generate_anchors -- said once, not silently
  static bool host_instead(const char *why) {
    static std::atomic<bool> said(false);
    if (!said.exchange(true)) fprintf(stderr, "\n[sedef_amd] seed anchors on the host for this input: %s\n", why);
    return false;
  }
  static bool short_enough(const std::vector<AnchorJob> &jobs) {
    for (const AnchorJob &j : jobs)
      if (j.query.size() >= (1u << 31) || j.ref.size() >= (1u << 31))
        return host_instead("GPU anchors implement sequences shorter than 2 Gb");
    return true;
  }
  static sdf_anchor_pair pair_at(const AnchorJob &j, int64_t q_off, int64_t r_off) {
    return {q_off, r_off, (int32_t)j.query.size(), (int32_t)j.ref.size(), j.same_chr, j.delta};
  }
  // the pairs as the device takes them: offsets of the pool_host() buffer when the driver fetched the sequences into it
  // (`in_pool`), else back to back (the caller copies them); `total`: the pool's extent
  void describe(const std::vector<AnchorJob> &jobs, std::vector<sdf_anchor_pair> &pairs, bool &in_pool, size_t &total) const {
    pairs.resize(jobs.size());
    total = 0;
    in_pool = pool_ != nullptr;
    for (size_t k = 0; k < jobs.size() && in_pool; k++)
      in_pool = jobs[k].query.data() >= pool_ && jobs[k].query.data() + jobs[k].query.size() <= pool_ + pool_cap_ &&
                jobs[k].ref.data() >= pool_ && jobs[k].ref.data() + jobs[k].ref.size() <= pool_ + pool_cap_;
    for (size_t k = 0; k < jobs.size(); k++) {
      const AnchorJob &j = jobs[k];
      const int64_t back_to_back = (int64_t)total;
      total += j.query.size() + j.ref.size();
      pairs[k] = in_pool ? pair_at(j, j.query.data() - pool_, j.ref.data() - pool_)
                         : pair_at(j, back_to_back, back_to_back + (int64_t)j.query.size());
    }
    if (in_pool) {  // (the pool's used extent, not the sum: slots are as long as the file's bytes, line ends included)
      total = 0;
      for (auto &pr : pairs) total = std::max<size_t>(total, (size_t)std::max(pr.q_off + pr.qlen, pr.r_off + pr.rlen));
    }
  }

  // generate_anchors on the device (include/sedef_hip.h: sdf_anchors_batch)
  bool anchors(const std::vector<AnchorJob> &jobs, int kmer, AnchorBatch &out) override {
    if (!stage_settings().gpu_anchors || jobs.empty()) return false;
    ready();  // (a reserve still running on its thread uses the context: its warm-up call, its pinning next to this upload)
    if (kmer > 15) return host_instead("GPU anchors implement k-mer sizes up to 15");
    if (!short_enough(jobs)) return false;
    if (genome_) return anchors_genome(jobs, kmer, false, 0, out);
    std::vector<sdf_anchor_pair> pairs;
    size_t total = 0;
    bool in_pool = false;
    describe(jobs, pairs, in_pool, total);
    // The characters of all pairs in the context's pinned staging (sized with the lane's other buffers) -- where the driver
    // fetched them, or copied there now --, one asynchronous DMA, and they STAY on the device: the DP rounds of this
    // super-batch name their tasks as ranges of them (run_resident).
    resident_ = false;
    char *pool = pool_;
    if (!in_pool) {
      pool = pool_ = sdf_pool_host(ctx_, total + 1);
      pool_cap_ = pool ? total + 1 : 0;
      uploaded_ = 0;
      if (!pool) return host_instead(sdf_last_error(ctx_));
      parallel_for((int)jobs.size(), [&](int k) {
        memcpy(pool + pairs[k].q_off, jobs[k].query.data(), jobs[k].query.size());
        memcpy(pool + pairs[k].r_off, jobs[k].ref.data(), jobs[k].ref.size());
      });
    }
    const auto tu0 = Clock::now();
    const bool sent = in_pool && uploaded_ >= total && sdf_pool_bytes(ctx_) >= total;  // (pool_ready() has sent it)
    if (!sent) {
      if (sdf_pool_upload(ctx_, pool, total) != SDF_OK) return host_instead(sdf_last_error(ctx_));
      uploaded_ = total;
      g_totals.chars += (long long)total;
    }
    if (stage_settings().debug_timing)
      fprintf(stderr, "[anchors: %zu pairs, pool %zu bytes %s, upload enqueued in %.1f ms]\n", jobs.size(), total,
              in_pool ? "fetched in place" : "copied", since(tu0) * 1e3);
    // (the anchors stay in the context's pinned staging: the jobs copy theirs out when they start)
    if (!anchors_call(pairs, nullptr, false, 0, std::max<size_t>(total, uploaded_), kmer, out)) return false;
    if (stage_settings().debug_timing)
      fprintf(stderr, "[anchors: device call returned %.1f ms after the upload was enqueued]\n", since(tu0) * 1e3);
    return true;
  }

  bool anchors_more(const std::vector<AnchorJob> &jobs, int kmer, size_t keep, AnchorBatch &out) override {
    if (!stage_settings().gpu_anchors || jobs.empty() || kmer > 15 || !(genome_ || (pool_ && uploaded_)) || !short_enough(jobs))
      return false;
    if (genome_) return anchors_genome(jobs, kmer, true, keep, out);
    std::vector<sdf_anchor_pair> pairs;
    size_t total = 0;
    bool in_pool = false;
    describe(jobs, pairs, in_pool, total);
    return in_pool && total <= uploaded_ && anchors_call(pairs, nullptr, true, keep, uploaded_, kmer, out);
  }

  // ---- resident chromosomes ----
  struct Genome {
    std::map<std::string, int64_t> base;  // record name -> pool offset of its base 0
  };
  bool has_genome() const override { return genome_ != nullptr; }
  bool chromosome_base(const std::string &name, int64_t *base_off) const override {
    if (!genome_) return false;
    const auto it = genome_->base.find(name);
    if (it == genome_->base.end()) return false;
    *base_off = it->second;
    return true;
  }
  bool load_genome(const FastaReference &fr, const std::vector<std::string> &names, size_t max_batch_bytes,
                   std::string &why) override {
    // every context first: its buffers sized and its warm-up calls -- which leave a small pool of their own -- over
    std::vector<GpuProvider *> all{this};
    join_spares();
    for (Spare &s : spares_)
      if (s.p) all.push_back(s.p.get());
    for (GpuProvider *g : all) {
      g->ready();
      if (!g->prepared_) {
        g->prepared_ = true;
        g->reserve(std::max<size_t>(max_batch_bytes, 1));
      }
      if (g->device_ != device_) {
        why = "the lanes are on several devices";
        return false;
      }
    }
    auto genome = std::make_shared<Genome>();
    long long chars = 0;
    for (const std::string &name : names) {
      const FastaReference::Record r = fr.record(name);
      int64_t at = 0;
      // (straight from the mapped file: no staged buffer is reused, one sdf_pool_sync below covers every record)
      const int rc = sdf_pool_append_fasta(ctx_, r.bytes, r.nbytes, r.entry->length, r.entry->line_blen, r.entry->line_len,
                                           genome->base.empty(), &at);
      if (rc != SDF_OK) {
        why = name + ": " + sdf_last_error(ctx_);
        return false;  // (what was appended so far goes with the next upload: it replaces the pool)
      }
      genome->base[name] = at;
      chars += r.entry->length;
    }
    if (genome->base.empty()) {
      why = "the buckets name no chromosome";
      return false;
    }
    if (sdf_pool_sync(ctx_) != SDF_OK) {
      why = sdf_last_error(ctx_);
      return false;
    }
    for (size_t i = 1; i < all.size(); i++)
      if (sdf_pool_share(all[i]->ctx_, ctx_) != SDF_OK) {
        why = sdf_last_error(all[i]->ctx_);
        // (all or nothing: the views made so far get a pool of their own again, so that the owner may replace its own)
        for (size_t j = 1; j < i; j++) (void)sdf_pool_upload(all[j]->ctx_, "N", 1);
        return false;
      }
    for (GpuProvider *g : all) g->genome_ = genome;
    g_totals.records += (long long)genome->base.size();
    g_totals.chars += chars;
    return true;
  }
  void plain_ranges(const int64_t *off, const int32_t *len, size_t n, char *plain) override {
    ready();
    std::vector<sdf_pool_range> ranges(n);
    for (size_t i = 0; i < n; i++) ranges[i] = {off[i], len[i], 0};
    std::vector<sdf_range_classes> cls(n);
    if (sdf_pool_range_classes(ctx_, ranges.data(), n, cls.data()) != SDF_OK)
      throw std::string("character classes of the resident pool failed: ") + sdf_last_error(ctx_);
    for (size_t i = 0; i < n; i++) plain[i] = cls[i].other == 0;
  }
  bool fetch_ranges(const int64_t *off, const int32_t *len, const char *rc, const size_t *dst_off, size_t n, char *dst,
                    size_t dst_bytes, std::string &why) override {
    ready();
    std::vector<sdf_pool_fetch> r(n);
    for (size_t i = 0; i < n; i++) r[i] = {off[i], len[i], rc[i] ? SDF_FETCH_RC : 0, (int64_t)dst_off[i]};
    if (sdf_pool_fetch_ranges(ctx_, r.data(), n, dst, dst_bytes) == SDF_OK) return true;
    why = sdf_last_error(ctx_);
    return false;
  }

 private:
  // the seed anchors of jobs that name ranges of the resident chromosomes: nothing is copied or uploaded
  bool anchors_genome(const std::vector<AnchorJob> &jobs, int kmer, bool more, size_t keep, AnchorBatch &out) {
    const size_t n = jobs.size();
    std::vector<sdf_anchor_pair> pairs(n);
    std::vector<uint8_t> strand(n);
    for (size_t k = 0; k < n; k++) {
      if (jobs[k].q_off < 0 || jobs[k].r_off < 0) throw std::string("internal: an anchor job without its resident ranges");
      pairs[k] = pair_at(jobs[k], jobs[k].q_off, jobs[k].r_off);
      strand[k] = jobs[k].r_rc;
    }
    return anchors_call(pairs, strand.data(), more, keep, sdf_pool_bytes(ctx_), kmer, out);
  }
  // One device call for the seed anchors of `pairs`, ranges of the `pool_bytes` characters on the device -- with a `strand`
  // byte per pair when they are ranges of the resident chromosomes; `more`: behind the `keep` anchors of the calls before,
  // which stay valid (false: no room behind them, or nothing the device covers -- the caller's ordinary call).
  bool anchors_call(const std::vector<sdf_anchor_pair> &pairs, const uint8_t *strand, bool more, size_t keep, size_t pool_bytes,
                    int kmer, AnchorBatch &out) {
    static_assert(sizeof(sdf_anchor) == sizeof(Anchor), "layouts must agree");
    const size_t n = pairs.size();
    out.off.assign(n + 1, 0);
    out.buf.reset();
    size_t used = 0;
    const sdf_anchor *found = nullptr;
    int rc;
    if (strand)
      rc = more ? sdf_anchors_batch_more_strand(ctx_, pairs.data(), strand, n, pool_bytes, kmer, keep, &found, out.off.data(), &used)
                : sdf_anchors_batch_view_strand(ctx_, pairs.data(), strand, n, nullptr, pool_bytes, kmer, &found, out.off.data(), &used);
    else
      rc = more ? sdf_anchors_batch_more(ctx_, pairs.data(), n, pool_bytes, kmer, keep, &found, out.off.data(), &used)
                : sdf_anchors_batch_view(ctx_, pairs.data(), n, nullptr, pool_bytes, kmer, &found, out.off.data(), &used);
    if (more && rc != SDF_OK) return false;
    if (rc == SDF_ERR_UNSUPPORTED || rc == SDF_ERR_NOMEM) return host_instead(sdf_last_error(ctx_));
    if (rc != SDF_OK) throw std::string("GPU anchors failed: ") + sdf_last_error(ctx_);
    out.view = (const Anchor *)found;
    // (the characters of an ordinary call stay in HBM for the DP rounds; resident chromosomes: load_stage_genome, never with
    // SDF_RESIDENT_DP=0)
    if (!more) resident_ = strand != nullptr || stage_settings().resident_dp;
    out.resident = resident_;
    out.q_base.resize(n);
    out.r_base.resize(n);
    for (size_t k = 0; k < n; k++) out.q_base[k] = pairs[k].q_off, out.r_base[k] = pairs[k].r_off;
    return true;
  }
  void join_spares() {
    for (Spare &s : spares_)
      if (s.starting.joinable()) s.starting.join();
  }
  std::shared_ptr<const Genome> genome_;  // the chromosomes in this context's pool (its own, or a view of the first lane's)
  sdf_ctx *ctx_;
  int device_;
  size_t ws_;
  int lanes_;
  bool prepared_ = false;
  bool resident_ = false;  // the last anchors() call's characters are in HBM (sdf_pool_upload)
  char *pool_ = nullptr;   // the context's pinned character staging as last asked for (pool_host / anchors)
  size_t uploaded_ = 0;    // bytes of it on the device (pool_ready / anchors)
  size_t pool_cap_ = 0;
  std::thread reserve_thread_;
  // the other lanes' providers: made side by side with this one (start_spares) or given back beyond those (give_back)
  struct Spare {
    std::unique_ptr<GpuProvider> p;  // (empty while a lane has it, or when its context could not be made)
    int device = 0;
    std::thread starting;
    bool taken = false;
  };
  std::vector<Spare> spares_;
  std::mutex spare_mu_;
};

struct OracleResult {  // layout of sdfo_result (oracle/extz2_oracle.h)
  uint32_t max;
  int32_t zdropped, max_q, max_t, mqe, mqe_t, mte, mte_q, score;
  int64_t n_cigar;
  uint32_t *cigar;
};

class TestProvider : public DpProvider {
 public:
  explicit TestProvider(test_dp_fn fn) : fn_(fn) {}
  void run(const std::vector<DpRequest> &reqs, const Params &p, Raw &raw) override {
    std::vector<TaskRef> tr;
    TaskPool pool;
    expand(reqs, p, tr, pool, raw.first_task);
    int8_t mat[25];
    fill_mat(p, mat);
    // the hook is re-entrant (like ksw_extz2_sse): tasks run on all host threads, their CIGAR words land in task order
    std::vector<OracleResult> res(tr.size());
    parallel_for((int)tr.size(), [&](int k) {
      const TaskRef &t = tr[(size_t)k];
      memset(&res[(size_t)k], 0, sizeof(OracleResult));
      fn_(t.qlen, pool.data() + t.q_off, t.tlen, pool.data() + t.t_off, 5, mat, -p.gap_open, -p.gap_extend, -1, -1,
          0, &res[(size_t)k]);
    });
    size_t words = 0;
    for (auto &r : res) words += (size_t)r.n_cigar;
    raw.own_recs.reset(new Raw::Rec[std::max<size_t>(tr.size(), 1)]);
    raw.own_words.reset(new uint32_t[std::max<size_t>(words, 1)]);
    words = 0;
    for (size_t k = 0; k < tr.size(); k++) {
      raw.own_recs[k] = {(int64_t)words, (int32_t)res[k].n_cigar, -1};  // (the oracle counts no matches)
      std::copy(res[k].cigar, res[k].cigar + res[k].n_cigar, raw.own_words.get() + words);
      words += (size_t)res[k].n_cigar;
      free(res[k].cigar);
      tasks++;
      cells += (int64_t)tr[k].qlen * tr[k].tlen;
    }
    raw.recs = raw.own_recs.get();
    raw.words = raw.own_words.get();
  }
  // (lanes of super-batches and of buckets work with the hook as with the device: the hook is re-entrant)
  std::unique_ptr<DpProvider> clone(int /*device*/ = -1) override { return std::unique_ptr<DpProvider>(new TestProvider(fn_)); }

 private:
  test_dp_fn fn_;
};

}  // namespace

size_t dp_chunks(int qlen, int tlen, size_t step, bool t_rc, int64_t t_off, long long *out, size_t cap) {
  return for_each_chunk(qlen, tlen, step, [&](size_t sp, int ql, int tl) {
    if (sp / step >= cap) return;
    long long *o = out + 4 * (sp / step);
    o[0] = (long long)sp, o[1] = chunk_target(t_off, tlen, sp, tl, t_rc), o[2] = ql, o[3] = tl;
  });
}

Cigar DpProvider::Raw::cigar(size_t req) const {
  Cigar c;
  c.matches = 0;
  for (size_t k = first_task[req]; k < first_task[req + 1]; k++) {
    append_ops(c, words + recs[k].off, recs[k].cnt);
    c.matches = c.matches < 0 || recs[k].match < 0 ? -1 : c.matches + recs[k].match;
  }
  return c;
}

std::vector<Cigar> DpProvider::run_cigars(const std::vector<DpRequest> &reqs, const Params &p) {
  Raw raw;
  run(reqs, p, raw);
  const auto t0 = Clock::now();
  std::vector<Cigar> out(reqs.size());
  for (size_t r = 0; r < reqs.size(); r++) out[r] = raw.cigar(r);
  t_unpack += since(t0);
  return out;
}

std::unique_ptr<DpProvider> make_gpu_provider(int device) { return std::unique_ptr<DpProvider>(new GpuProvider(device)); }

std::unique_ptr<DpProvider> make_gpu_providers(int device, int lanes, const std::vector<int> &devices, size_t max_batch_bytes) {
  return std::unique_ptr<DpProvider>(new GpuProvider(device, std::max(lanes - 1, 0), devices, max_batch_bytes));
}

std::unique_ptr<DpProvider> make_test_provider(test_dp_fn fn) { return std::unique_ptr<DpProvider>(new TestProvider(fn)); }

}  // namespace sdfh
