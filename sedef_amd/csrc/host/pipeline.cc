// fast_align + refine_chains as a resumable per-pair job, the DP providers, and the stage driver
// (restates reference src/chain.cc:203-268, src/refine.cc:23-193, src/align_main.cc:200-337).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <fstream>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <future>
#include <mutex>
#include <set>
#include <thread>

#include "../../../include/sedef_hip.h"
#include <dirent.h>
#include <sys/stat.h>

#include "sedef_host.h"

namespace sdfh {

void set_alignment_scoring(const Params &p);

namespace {
struct StageTotals {
  std::atomic<long long> records{0}, chars{0}, batches{0}, batches_resident{0};
} g_totals;
}  // namespace
void stage_totals_reset() { g_totals.records = g_totals.chars = g_totals.batches = g_totals.batches_resident = 0; }
void stage_totals(long long out[4]) {
  out[0] = g_totals.records, out[1] = g_totals.chars, out[2] = g_totals.batches, out[3] = g_totals.batches_resident;
}

bool resident_range(int64_t base, int64_t start, int64_t seq_len, int64_t s, int64_t len, bool rc, int64_t *off) {
  if (s < 0 || len < 0 || seq_len < 0 || s > seq_len || len > seq_len - s) return false;
  *off = rc ? base + start + seq_len - s - len : base + start + s;
  return true;
}
static void parallel_for(int n, const std::function<void(int)> &body);  // all host cores (defined below)

// ======================================================================================================
// DP providers: align_helper (src/align.cc:39-68) for a batch of requests
// ======================================================================================================
namespace {

struct TaskRef {
  size_t req;
  size_t q_off, t_off;
  int qlen, tlen;
};

// chunking of one request into DP tasks (src/align.cc:46-57): both sequences advance by the same SP.
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
  const size_t n = reqs.size(), step = (size_t)p.max_ksw_seq_len;
  std::vector<size_t> off(n + 1, 0);
  first.assign(n + 1, 0);
  for (size_t k = 0; k < n; k++) {
    const DpRequest &r = reqs[k];
    off[k + 1] = off[k] + (size_t)r.qlen + (size_t)r.tlen;
    const size_t lim = (size_t)std::min(r.qlen, r.tlen);
    first[k + 1] = first[k] + (lim + step - 1) / step;
  }
  pool.size = off[n];
  pool.bytes.reset(new uint8_t[std::max<size_t>(off[n], 1)]);
  tasks.resize(first[n]);
  const size_t block = 4096;
  parallel_for((int)((n + block - 1) / block), [&](int b) {
    for (size_t k = (size_t)b * block; k < std::min(n, ((size_t)b + 1) * block); k++) {
      const DpRequest &r = reqs[k];
      const size_t qo = off[k], to = qo + (size_t)r.qlen;
      uint8_t *dq = pool.bytes.get() + qo, *dt = pool.bytes.get() + to;
      for (int i = 0; i < r.qlen; i++) dq[i] = kCodes.of[(unsigned char)r.q[i]];
      for (int i = 0; i < r.tlen; i++) dt[i] = kCodes.of[(unsigned char)r.t[i]];
      const size_t lim = (size_t)std::min(r.qlen, r.tlen);
      size_t at = first[k];
      for (size_t sp = 0; sp < lim; sp += step) {
        TaskRef &t = tasks[at++];
        t.req = k;
        t.q_off = qo + sp;
        t.t_off = to + sp;
        t.qlen = (int)std::min<size_t>(step, (size_t)r.qlen - sp);
        t.tlen = (int)std::min<size_t>(step, (size_t)r.tlen - sp);
      }
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
      for (auto &t : spare_threads_)
        if (t.joinable()) t.join();
      throw std::string("GPU DP backend unavailable: ") + sdf_last_error(nullptr);
    }
    if (max_batch_bytes) {
      prepared_ = true;
      reserve(max_batch_bytes);
    }
  }
  ~GpuProvider() override {
    ready();
    for (auto &t : spare_threads_)
      if (t.joinable()) t.join();
    {  // (the spare lanes' device contexts side by side: a context takes 30-40 ms to give back)
      std::vector<std::thread> gone;
      for (auto &e : spares_)
        if (e) gone.emplace_back([&e] { e.reset(); });
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
    spare_dev_.resize((size_t)n);
    for (int i = 0; i < n; i++) {
      spare_dev_[(size_t)i] = devices.empty() ? device_ : devices[(size_t)(i + 1) % devices.size()];
      spare_threads_.emplace_back([this, i, n, max_batch_bytes] {
        try {
          spares_[(size_t)i].reset(new GpuProvider(spare_dev_[(size_t)i], 0, std::vector<int>(), max_batch_bytes, n + 1));
        } catch (...) {  // (no room for another context: clone() will try again, the lane does without)
        }
      });
    }
  }
  std::unique_ptr<DpProvider> clone(int device = -1) override {
    const int want = device < 0 ? device_ : device;
    {
      std::lock_guard<std::mutex> g(spare_mu_);
      for (size_t i = 0; i < spares_.size(); i++) {
        if (spare_dev_[i] != want || spare_taken_.count(i)) continue;
        spare_taken_.insert(i);
        if (spare_threads_[i].joinable()) spare_threads_[i].join();
        if (spares_[i]) return std::unique_ptr<DpProvider>(spares_[i].release());
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
    for (size_t i = 0; i < spares_.size(); i++)
      if (spare_taken_.count(i) && !spares_[i] && spare_dev_[i] == g->device_) {
        p.release();
        spares_[i].reset(g);
        spare_taken_.erase(i);
        return;
      }
    p.release();  // (made by clone() beyond the spares the provider started with: one more place)
    spares_.emplace_back(g);
    spare_dev_.push_back(g->device_);
    spare_threads_.emplace_back();
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
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = sdf_reserve(ctx_, tasks, bases, ws_, SDF_RESERVE_BRIEF | SDF_RESERVE_ANCHORS | (lanes_ > 1 ? SDF_RESERVE_FEW_STREAMS : 0u));
    // (the super-batch's characters are written straight into pinned memory and cross PCIe as one DMA: sized here, once)
    // (a sequence's slot is as long as its range in the FILE -- a line end per 50-80 bases --, and a pair's end may move to the
    // chromosome's: a sixteenth more than the bases, so that the stage never pins a second time)
    if (stage_settings().gpu_anchors) (void)sdf_pool_host(ctx_, max_batch_bytes + max_batch_bytes / 16 + (1u << 20));
    if (stage_settings().debug_timing)
      fprintf(stderr, "[sdf_reserve tasks %zu bases %zu: rc %d, %.1f ms]\n", tasks, bases, rc,
              std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
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
    const auto tp0 = std::chrono::steady_clock::now();
    expand(reqs, p, tr, pool, raw.first_task);
    if (tr.empty()) return;
    const size_t nt = tr.size();
    std::unique_ptr<sdf_task[]> tasks(new sdf_task[nt]);
    const size_t tblock = 16384, ntb = (nt + tblock - 1) / tblock;
    parallel_for((int)ntb, [&](int b) {
      for (size_t k = (size_t)b * tblock; k < std::min(nt, ((size_t)b + 1) * tblock); k++)
        tasks[k] = make_task((int64_t)tr[k].q_off, (int64_t)tr[k].t_off, tr[k].qlen, tr[k].tlen);
    });
    call_batch(tasks.get(), nt, &pool, p, raw, tp0);
  }

  // The same round on ranges of the character pool the last anchors() call left on the device: nothing is cut out, coded,
  // packed or uploaded here (include/sedef_hip.h: sdf_extz2_batch_pairs) -- a request becomes its 60 kb chunks
  // (src/align.cc:46-47: both sequences advance by the same offset) and that is all the host does per task.
  bool run_resident(const std::vector<ResidentReq> &reqs, const Params &p, Raw &raw) override {
    if (!resident_) return false;
    const size_t n = reqs.size(), step = (size_t)p.max_ksw_seq_len;
    raw.first_task.assign(n + 1, 0);
    raw.recs = nullptr;
    raw.words = nullptr;
    if (reqs.empty()) return true;
    const auto tp0 = std::chrono::steady_clock::now();
    const size_t rblock = 16384, nrb = (n + rblock - 1) / rblock;
    std::vector<size_t> bfirst(nrb + 1, 0);
    parallel_for((int)nrb, [&](int b) {
      size_t c = 0;
      for (size_t k = (size_t)b * rblock; k < std::min(n, ((size_t)b + 1) * rblock); k++)
        c += ((size_t)std::min(reqs[k].qlen, reqs[k].tlen) + step - 1) / step;
      bfirst[(size_t)b + 1] = c;
    });
    for (size_t b = 0; b < nrb; b++) bfirst[b + 1] += bfirst[b];
    const size_t nt = bfirst[nrb];
    raw.first_task[n] = nt;
    if (nt == 0) {
      std::fill(raw.first_task.begin(), raw.first_task.end(), 0);
      return true;
    }
    std::unique_ptr<sdf_task[]> tasks(new sdf_task[nt]);
    parallel_for((int)nrb, [&](int b) {
      size_t at = bfirst[(size_t)b];
      for (size_t k = (size_t)b * rblock; k < std::min(n, ((size_t)b + 1) * rblock); k++) {
        const ResidentReq &r = reqs[k];
        raw.first_task[k] = at;
        const size_t lim = (size_t)std::min(r.qlen, r.tlen);
        for (size_t sp = 0; sp < lim; sp += step) {
          const int ql = (int)std::min<size_t>(step, (size_t)r.qlen - sp), tl = (int)std::min<size_t>(step, (size_t)r.tlen - sp);
          // (a reversed target is read from the END of its range: chunk sp holds its bases [sp, sp + tl))
          const int64_t to = (r.flag & SDF_TASK_T_RC) ? r.t_off + r.tlen - (int64_t)sp - tl : r.t_off + (int64_t)sp;
          tasks[at++] = make_task(r.q_off + (int64_t)sp, to, ql, tl, r.flag);
        }
      }
    });
    call_batch(tasks.get(), nt, nullptr, p, raw, tp0);
    return true;
  }

 private:
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
  void call_batch(const sdf_task *tasks, size_t nt, const TaskPool *pool, const Params &p, Raw &raw,
                  std::chrono::steady_clock::time_point tp0) {
    const size_t tblock = 16384, ntb = (nt + tblock - 1) / tblock;
    std::vector<size_t> cap_part(ntb, 0);
    std::vector<int64_t> cells_part(ntb, 0);
    parallel_for((int)ntb, [&](int b) {
      size_t cap_b = 0;
      int64_t cells_b = 0;
      for (size_t k = (size_t)b * tblock; k < std::min(nt, ((size_t)b + 1) * tblock); k++) {
        cap_b += (size_t)tasks[k].qlen + tasks[k].tlen + 2;
        cells_b += (int64_t)tasks[k].qlen * tasks[k].tlen;
      }
      cap_part[(size_t)b] = cap_b;
      cells_part[(size_t)b] = cells_b;
    });
    size_t cap = 0;
    for (size_t b = 0; b < ntb; b++) cap += cap_part[b], cells += cells_part[b];
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
    const auto tp1 = std::chrono::steady_clock::now();
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
    const auto tp2 = std::chrono::steady_clock::now();
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
  // the pairs as the device takes them: offsets of the pool_host() buffer when the driver fetched the sequences into it
  // (`in_pool`), else back to back (the caller copies them); `total`: the pool's extent
  bool describe(const std::vector<AnchorJob> &jobs, std::vector<sdf_anchor_pair> &pairs, bool &in_pool, size_t &total) const {
    pairs.resize(jobs.size());
    total = 0;
    in_pool = pool_ != nullptr;
    for (size_t k = 0; k < jobs.size() && in_pool; k++)
      in_pool = jobs[k].query.data() >= pool_ && jobs[k].query.data() + jobs[k].query.size() <= pool_ + pool_cap_ &&
                jobs[k].ref.data() >= pool_ && jobs[k].ref.data() + jobs[k].ref.size() <= pool_ + pool_cap_;
    for (size_t k = 0; k < jobs.size(); k++) {
      if (jobs[k].query.size() >= (1u << 31) || jobs[k].ref.size() >= (1u << 31))
        return host_instead("GPU anchors implement sequences shorter than 2 Gb");
      pairs[k].q_off = in_pool ? (int64_t)(jobs[k].query.data() - pool_) : (int64_t)total;
      total += jobs[k].query.size();
      pairs[k].r_off = in_pool ? (int64_t)(jobs[k].ref.data() - pool_) : (int64_t)total;
      total += jobs[k].ref.size();
      pairs[k].qlen = (int32_t)jobs[k].query.size();
      pairs[k].rlen = (int32_t)jobs[k].ref.size();
      pairs[k].same_chr = jobs[k].same_chr;
      pairs[k].delta = jobs[k].delta;
    }
    if (in_pool) {  // (the pool's used extent, not the sum: slots are as long as the file's bytes, line ends included)
      total = 0;
      for (auto &pr : pairs) total = std::max<size_t>(total, (size_t)std::max(pr.q_off + pr.qlen, pr.r_off + pr.rlen));
    }
    return true;
  }
  void describe_out(const std::vector<sdf_anchor_pair> &pairs, AnchorBatch &out) const {
    out.resident = resident_;
    out.q_base.resize(pairs.size());
    out.r_base.resize(pairs.size());
    for (size_t k = 0; k < pairs.size(); k++) out.q_base[k] = pairs[k].q_off, out.r_base[k] = pairs[k].r_off;
  }

  // generate_anchors on the device (include/sedef_hip.h: sdf_anchors_batch)
  bool anchors(const std::vector<AnchorJob> &jobs, int kmer, AnchorBatch &out) override {
    if (!stage_settings().gpu_anchors || jobs.empty()) return false;
    ready();  // (a reserve still running on its thread uses the context: its warm-up call, its pinning next to this upload)
    if (kmer > 15) return host_instead("GPU anchors implement k-mer sizes up to 15");
    if (genome_) return anchors_genome(jobs, kmer, false, 0, out);
    std::vector<sdf_anchor_pair> pairs;
    size_t total = 0;
    bool in_pool = false;
    if (!describe(jobs, pairs, in_pool, total)) return false;
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
    const auto tu0 = std::chrono::steady_clock::now();
    const bool sent = in_pool && uploaded_ >= total && sdf_pool_bytes(ctx_) >= total;  // (pool_ready() has sent it)
    if (!sent) {
      if (sdf_pool_upload(ctx_, pool, total) != SDF_OK) return host_instead(sdf_last_error(ctx_));
      uploaded_ = total;
      g_totals.chars += (long long)total;
    }
    if (stage_settings().debug_timing)
      fprintf(stderr, "[anchors: %zu pairs, pool %zu bytes %s, upload enqueued in %.1f ms]\n", jobs.size(), total,
              in_pool ? "fetched in place" : "copied", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tu0).count());
    out.off.assign(jobs.size() + 1, 0);
    size_t used = 0;
    static_assert(sizeof(sdf_anchor) == sizeof(Anchor), "layouts must agree");
    // (the anchors stay in the context's pinned staging: the jobs copy theirs out when they start)
    const sdf_anchor *found = nullptr;
    out.buf.reset();
    int rc = sdf_anchors_batch_view(ctx_, pairs.data(), pairs.size(), nullptr, std::max<size_t>(total, uploaded_), kmer, &found,
                                    out.off.data(), &used);
    out.view = (const Anchor *)found;
    if (rc == SDF_ERR_UNSUPPORTED || rc == SDF_ERR_NOMEM) return host_instead(sdf_last_error(ctx_));
    if (rc != SDF_OK) throw std::string("GPU anchors failed: ") + sdf_last_error(ctx_);
    if (stage_settings().debug_timing)
      fprintf(stderr, "[anchors: device call returned %.1f ms after the upload was enqueued]\n",
              std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tu0).count());
    resident_ = stage_settings().resident_dp;
    describe_out(pairs, out);
    return true;
  }

  bool anchors_more(const std::vector<AnchorJob> &jobs, int kmer, size_t keep, AnchorBatch &out) override {
    if (genome_) return stage_settings().gpu_anchors && !jobs.empty() && kmer <= 15 && anchors_genome(jobs, kmer, true, keep, out);
    if (!stage_settings().gpu_anchors || jobs.empty() || kmer > 15 || !pool_ || !uploaded_) return false;
    std::vector<sdf_anchor_pair> pairs;
    size_t total = 0;
    bool in_pool = false;
    if (!describe(jobs, pairs, in_pool, total) || !in_pool || total > uploaded_) return false;
    out.off.assign(jobs.size() + 1, 0);
    size_t used = 0;
    const sdf_anchor *found = nullptr;
    out.buf.reset();
    const int rc = sdf_anchors_batch_more(ctx_, pairs.data(), pairs.size(), uploaded_, kmer, keep, &found, out.off.data(), &used);
    if (rc != SDF_OK) return false;  // (no room behind the kept anchors, or nothing the device covers: the caller's fallback)
    out.view = (const Anchor *)found;
    describe_out(pairs, out);
    return true;
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
    for (auto &t : spare_threads_)
      if (t.joinable()) t.join();
    for (auto &e : spares_)
      if (e) all.push_back(e.get());
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
      if (jobs[k].query.size() >= (1u << 31) || jobs[k].ref.size() >= (1u << 31))
        return host_instead("GPU anchors implement sequences shorter than 2 Gb");
      pairs[k] = {jobs[k].q_off, jobs[k].r_off, (int32_t)jobs[k].query.size(), (int32_t)jobs[k].ref.size(), jobs[k].same_chr,
                  jobs[k].delta};
      strand[k] = jobs[k].r_rc;
    }
    out.off.assign(n + 1, 0);
    out.buf.reset();
    size_t used = 0;
    const sdf_anchor *found = nullptr;
    const size_t pool_bytes = sdf_pool_bytes(ctx_);
    const int rc = more ? sdf_anchors_batch_more_strand(ctx_, pairs.data(), strand.data(), n, pool_bytes, kmer, keep, &found,
                                                        out.off.data(), &used)
                        : sdf_anchors_batch_view_strand(ctx_, pairs.data(), strand.data(), n, nullptr, pool_bytes, kmer, &found,
                                                        out.off.data(), &used);
    if (more && rc != SDF_OK) return false;  // (no room behind the kept anchors: the caller's ordinary call)
    if (rc == SDF_ERR_UNSUPPORTED || rc == SDF_ERR_NOMEM) return host_instead(sdf_last_error(ctx_));
    if (rc != SDF_OK) throw std::string("GPU anchors failed: ") + sdf_last_error(ctx_);
    out.view = (const Anchor *)found;
    resident_ = true;  // (load_stage_genome: never with SDF_RESIDENT_DP=0)
    describe_out(pairs, out);
    return true;
  }
  std::shared_ptr<const Genome> genome_;  // the chromosomes in this context's pool (its own, or a view of the first lane's)
  sdf_ctx *ctx_;
  int device_;
  size_t ws_;
  int lanes_;
  int64_t tasks_ = 0;
  bool prepared_ = false;
  bool resident_ = false;  // the last anchors() call's characters are in HBM (sdf_pool_upload)
  char *pool_ = nullptr;   // the context's pinned character staging as last asked for (pool_host / anchors)
  size_t uploaded_ = 0;    // bytes of it on the device (pool_ready / anchors)
  size_t pool_cap_ = 0;
  std::thread reserve_thread_;
  std::vector<std::unique_ptr<GpuProvider>> spares_;
  std::vector<int> spare_dev_;
  std::vector<std::thread> spare_threads_;
  std::set<size_t> spare_taken_;
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
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<Cigar> out(reqs.size());
  for (size_t r = 0; r < reqs.size(); r++) out[r] = raw.cigar(r);
  t_unpack += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return out;
}

std::unique_ptr<DpProvider> make_gpu_provider(int device) { return std::unique_ptr<DpProvider>(new GpuProvider(device)); }

std::unique_ptr<DpProvider> make_gpu_providers(int device, int lanes, const std::vector<int> &devices, size_t max_batch_bytes) {
  return std::unique_ptr<DpProvider>(new GpuProvider(device, std::max(lanes - 1, 0), devices, max_batch_bytes));
}

static int stage_super_batch(int total, int nlanes, int super_batch) {
  if (nlanes > 1) super_batch = std::max(1024, std::min(super_batch, (total + 2 * nlanes - 1) / (2 * nlanes)));
  if (stage_settings().super_batch > 0) super_batch = stage_settings().super_batch;
  return super_batch;
}

StageHint stage_hint(const std::string &bed_path, int super_batch) {
  StageHint h;
  std::vector<int64_t> bytes;
  if (FILE *f = fopen(bed_path.c_str(), "rb")) {
    // columns 2, 3 and 5, 6 of a line: the two intervals (src/hit.cc: Hit::from_bed); anything else is skipped
    std::vector<char> line(1 << 16);
    while (fgets(line.data(), (int)line.size(), f)) {
      int64_t v[6] = {0, 0, 0, 0, 0, 0};
      int col = 0;
      for (const char *c = line.data(); *c && *c != '\n' && col < 6; ++col) {
        const char *e = c;
        while (*e && *e != '\t' && *e != '\n') ++e;
        if (col == 1 || col == 2 || col == 4 || col == 5) v[col] = atoll(c);
        c = *e == '\t' ? e + 1 : e;
      }
      bytes.push_back(std::max<int64_t>(0, v[2] - v[1]) + std::max<int64_t>(0, v[5] - v[4]));
    }
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
std::unique_ptr<DpProvider> make_test_provider(test_dp_fn fn) { return std::unique_ptr<DpProvider>(new TestProvider(fn)); }

// ======================================================================================================
// PairJob
// ======================================================================================================
namespace {
std::atomic<long long> g_us_chain(0), g_us_rest(0);  // host CPU time (summed over threads), microseconds
struct ScopedUs {
  std::atomic<long long> &acc;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  explicit ScopedUs(std::atomic<long long> &a) : acc(a) {}
  ~ScopedUs() { acc += std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count(); }
};
}  // namespace

struct PairJob::PathState {
  std::deque<int> idx;       // chain hits of the path, in order
  int qlo, qhi, rlo, rhi;    // extent from the chain coordinates (before any merge)
  bool est_ok = true;
  // progress
  size_t pi = 1;
  int prev = -1;             // index into hits_
  std::vector<Hit> guide;
  bool merging = false;      // waiting for the gap DP of a merge
  bool building = false;     // waiting for the DPs of the final guide alignment
  bool finished = false;
  Hit result;
};

PairJob::PairJob(SeqView query, SeqView ref, const Hit &orig, const Params &p, bool scan)
    : query_(query), ref_(ref), orig_(orig), p_(p) {
  if (!scan) return;
  auto plain = [](SeqView s) {
    static const struct Tab {
      bool ok[256];
      Tab() {
        for (auto &b : ok) b = false;
        for (const char *c = "ACGTNacgtn"; *c; ++c) ok[(unsigned char)*c] = true;
      }
    } tab;
    for (unsigned char c : s)
      if (!tab.ok[c]) return false;
    return true;
  };
  exact_ = plain(query) && plain(ref);
}

void PairJob::stage_start(std::vector<DpRequest> &out) {  // src/chain.cc:203-258
  // (the hits' Sequence objects carry names and strands; nothing of the stage reads bases through them -- a copy of both
  // sequences per pair was 182 MB of memcpy and page faults in the chr1-sized run)
  query_ptr_ = std::make_shared<Sequence>("QRY", std::string());
  ref_ptr_ = std::make_shared<Sequence>("REF", std::string());
  if (!have_anchors_) anchors_ = generate_anchors(query_.str(), ref_.str(), orig_, p_.kmer);
  else anchors_.assign(ext_anchors_, ext_anchors_ + ext_count_);
  auto chains = chain_anchors(anchors_, p_);
  const auto &chain = chains.first;
  const auto &bounds = chains.second;
  const double min_span = p_.min_read_size * (1 - p_.max_error);
  for (size_t bi = 1; bi < bounds.size(); bi++) {
    const bool has_u = bounds[bi].second;
    const int be = bounds[bi].first, bs = bounds[bi - 1].first;
    const int up = bounds[bi].second;
    const int qlo = anchors_[chain[be - 1]].q, qhi = anchors_[chain[bs]].q + anchors_[chain[bs]].l;
    const int rlo = anchors_[chain[be - 1]].r, rhi = anchors_[chain[bs]].r + anchors_[chain[bs]].l;
    const int span = std::max(rhi - rlo, qhi - qlo);
    if ((!has_u || span < p_.min_uppercase_match) && span < min_span) continue;
    Hit a;
    a.query = query_ptr_;
    a.query_start = qlo;
    a.query_end = qhi;
    a.ref = ref_ptr_;
    a.ref_start = rlo;
    a.ref_end = rhi;
    a.jaccard = up;
    guides_.push_back(std::vector<int>());
    for (int k = be - 1; k >= bs; k--) guides_.back().push_back(chain[k]);
    hits_.push_back(a);
  }
  DpSession rec;
  rec.recording = true;
  rec.requests = &out;
  for (size_t k = 0; k < hits_.size(); k++) Alignment tmp(query_, ref_, anchors_, guides_[k], rec);
}

void PairJob::stage_chain_finish(const std::vector<Cigar> &results) {
  DpSession rep;
  rep.recording = false;
  rep.results = &results;
  rep.codes_are_exact = exact_;
  for (size_t k = 0; k < hits_.size(); k++) {
    hits_[k].aln = Alignment(query_, ref_, anchors_, guides_[k], rep);
    update_from_alignment(hits_[k]);
  }
  std::vector<Anchor>().swap(anchors_);
  plan_paths();
}

void PairJob::plan_paths() {  // src/refine.cc:23-147
  std::vector<Hit> &anchors = hits_;
  std::sort(anchors.begin(), anchors.end());
  const bool same_chr = orig_.query->name == orig_.ref->name && orig_.query->is_rc == orig_.ref->is_rc;
  std::vector<int> score;
  for (auto &a : anchors)
    score.push_back(p_.refine_match * a.aln.matches() - p_.refine_mismatch * a.aln.mismatches() -
                    p_.refine_gap * a.aln.gap_bases());  // double -> int
  std::vector<int> dp(anchors.size(), 0), prev(anchors.size(), -1);
  std::set<std::pair<int, int>, std::greater<std::pair<int, int>>> maxes;
  for (int ai = 0; ai < (int)anchors.size(); ai++) {
    if (same_chr) {
      auto &c = anchors[ai];
      const int qlo = c.query_start, qhi = c.query_end, rlo = c.ref_start, rhi = c.ref_end;
      const int qo = std::max(0, std::min(orig_.query_start + qhi, orig_.ref_start + rhi) -
                                     std::max(orig_.query_start + qlo, orig_.ref_start + rlo));
      if ((rhi - rlo) - qo < p_.refine_side_align && (qhi - qlo) - qo < p_.refine_side_align) continue;
    }
    dp[ai] = score[ai];
    for (int aj = ai - 1; aj >= 0; aj--) {
      auto &c = anchors[ai];
      auto &p = anchors[aj];
      int cqs = c.query_start;
      if (cqs < p.query_end) cqs = p.query_end;
      int crs = c.ref_start;
      if (crs < p.ref_end) crs = p.ref_end;
      if (p.query_end >= c.query_end || p.ref_end >= c.ref_end) continue;
      if (p.ref_start >= c.ref_start) continue;
      const int ma = std::max(cqs - p.query_end, crs - p.ref_end);
      const int mi = std::min(cqs - p.query_end, crs - p.ref_end);
      if (ma >= p_.refine_max_gap) continue;
      if (same_chr) {
        const int qlo = p.query_end, qhi = cqs, rlo = p.ref_end, rhi = crs;
        const int qo = std::max(0, std::min(orig_.query_start + qhi, orig_.ref_start + rhi) -
                                       std::max(orig_.query_start + qlo, orig_.ref_start + rlo));
        if (qo >= 1) continue;
      }
      const int mis = p_.refine_mismatch * mi, gap = p_.refine_gapopen + p_.refine_gap * (ma - mi);
      const int sco = dp[aj] + score[ai] - mis - gap;
      if (sco >= dp[ai]) {
        dp[ai] = sco;
        prev[ai] = aj;
      }
    }
    maxes.insert({dp[ai], ai});
  }
  std::vector<bool> used(anchors.size(), false);
  for (auto &m : maxes) {
    if (m.first == 0) break;
    int maxi = m.second;
    if (used[maxi]) continue;
    auto ps = std::make_shared<PathState>();
    while (maxi != -1 && !used[maxi]) {
      ps->idx.push_front(maxi);
      used[maxi] = true;
      maxi = prev[maxi];
    }
    ps->qlo = anchors[ps->idx.front()].query_start;
    ps->qhi = anchors[ps->idx.back()].query_end;
    ps->rlo = anchors[ps->idx.front()].ref_start;
    ps->rhi = anchors[ps->idx.back()].ref_end;
    int est_size = anchors[ps->idx[0]].aln.span();
    for (size_t i = 1; i < ps->idx.size(); i++) {
      est_size += anchors[ps->idx[i]].aln.span();
      est_size += std::max(anchors[ps->idx[i]].query_start - anchors[ps->idx[i - 1]].query_end,
                           anchors[ps->idx[i]].ref_start - anchors[ps->idx[i - 1]].ref_end);
    }
    ps->est_ok = est_size >= p_.refine_min_read - p_.refine_side_align;
    ps->prev = ps->idx[0];
    paths_.push_back(ps);
  }
}

std::vector<DpRequest> PairJob::advance(const std::vector<Cigar> &results) {
  std::vector<DpRequest> out;
  ScopedUs timer(stage_ == START ? g_us_chain : g_us_rest);
  if (stage_ == START) {
    stage_start(out);
    stage_ = CHAIN_ALN;
    if (!out.empty()) return out;
    // no DP needed: fall through with an empty result set
    stage_chain_finish(std::vector<Cigar>());
    stage_ = PATHS;
  } else if (stage_ == CHAIN_ALN) {
    stage_chain_finish(results);
    stage_ = PATHS;
  }
  if (stage_ != PATHS) return out;

  // distribute the results of the previous round to the paths that were waiting, in request order
  size_t cursor = 0;
  std::vector<int> waiting;
  waiting.swap(wait_paths_);
  std::vector<size_t> counts;
  counts.swap(wait_counts_);
  std::vector<std::vector<Cigar>> path_results(paths_.size());
  for (size_t w = 0; w < waiting.size(); w++) {
    path_results[waiting[w]].assign(results.begin() + cursor, results.begin() + cursor + counts[w]);
    cursor += counts[w];
  }

  const SeqView qseq = query_, rseq = ref_;
  for (size_t pk = 0; pk < paths_.size(); pk++) {
    PathState &ps = *paths_[pk];
    if (ps.finished || !ps.est_ok) continue;
    std::vector<Cigar> have;
    have.swap(path_results[pk]);
    bool have_results = ps.merging || ps.building;
    for (;;) {
      if (ps.building) {  // results of the final guide alignment are here
        DpSession rep;
        rep.recording = false;
        rep.results = &have;
        rep.codes_are_exact = exact_;
        ps.result.aln = Alignment(qseq, rseq, ps.guide, p_.refine_side_align, rep);
        update_from_alignment(ps.result);
        ps.finished = true;
        break;
      }
      if (ps.merging) {  // results of a merge's gap DP are here: do the real merge
        Hit &prev = hits_[ps.prev];
        Hit &cur = hits_[ps.idx[ps.pi]];
        DpSession rep;
        rep.recording = false;
        rep.results = &have;
        rep.codes_are_exact = exact_;
        prev.aln.merge(cur.aln, qseq, rseq, rep);
        update_from_alignment(prev);
        ps.merging = false;
        ps.pi++;
        have.clear();
        have_results = false;
      }
      // walk the path (src/refine.cc:165-179)
      bool waiting_now = false;
      while (ps.pi < ps.idx.size()) {
        Hit &prev = hits_[ps.prev];
        Hit &cur = hits_[ps.idx[ps.pi]];
        if (cur.query_start < prev.query_end || cur.ref_start < prev.ref_end) {
          // enumerate the merge's DP request on copies
          std::vector<DpRequest> reqs;
          DpSession rec;
          rec.recording = true;
          rec.requests = &reqs;
          Alignment pa = prev.aln, ca = cur.aln;
          pa.merge(ca, qseq, rseq, rec);
          if (reqs.empty()) {
            std::vector<Cigar> none;
            DpSession rep;
            rep.recording = false;
            rep.results = &none;
            rep.codes_are_exact = exact_;
            prev.aln.merge(cur.aln, qseq, rseq, rep);
            update_from_alignment(prev);
            ps.pi++;
            continue;
          }
          ps.merging = true;
          wait_paths_.push_back((int)pk);
          wait_counts_.push_back(reqs.size());
          out.insert(out.end(), reqs.begin(), reqs.end());
          waiting_now = true;
          break;
        }
        ps.guide.push_back(prev);
        ps.prev = ps.idx[ps.pi];
        ps.pi++;
      }
      if (waiting_now) break;
      // end of the path: the refined hit (src/refine.cc:163,180-183)
      ps.guide.push_back(hits_[ps.prev]);
      ps.result = Hit();
      ps.result.query = hits_.front().query;
      ps.result.query_start = ps.qlo;
      ps.result.query_end = ps.qhi;
      ps.result.ref = hits_.front().ref;
      ps.result.ref_start = ps.rlo;
      ps.result.ref_end = ps.rhi;
      std::vector<DpRequest> reqs;
      DpSession rec;
      rec.recording = true;
      rec.requests = &reqs;
      { Alignment tmp(qseq, rseq, ps.guide, p_.refine_side_align, rec); }
      ps.building = true;
      if (reqs.empty()) {
        have.clear();
        continue;  // build immediately
      }
      wait_paths_.push_back((int)pk);
      wait_counts_.push_back(reqs.size());
      out.insert(out.end(), reqs.begin(), reqs.end());
      break;
    }
    (void)have_results;
  }
  if (out.empty()) {
    finish_paths();
    stage_ = DONE;
  }
  return out;
}

void PairJob::finish_paths() {  // acceptance replay: src/refine.cc:143-162,184-190
  for (auto &pp : paths_) {
    PathState &ps = *pp;
    if (!ps.est_ok) continue;
    bool overlap = false;
    for (auto &h : final_hits_) {
      const int qo = std::max(0, std::min(ps.qhi, h.query_end) - std::max(ps.qlo, h.query_start));
      const int ro = std::max(0, std::min(ps.rhi, h.ref_end) - std::max(ps.rlo, h.ref_start));
      if (ps.qhi - ps.qlo - qo < p_.refine_side_align && ps.rhi - ps.rlo - ro < p_.refine_side_align) {
        overlap = true;
        break;
      }
    }
    if (overlap) continue;
    if (ps.result.aln.span() >= p_.refine_min_read) final_hits_.push_back(ps.result);
  }
  paths_.clear();
  hits_.clear();
}

// ======================================================================================================
// Stage driver
// ======================================================================================================
// The per-pair host work (anchors, chaining, refinement, CIGAR algebra) is independent across pairs: run it on
// all host cores (SDF_HOST_THREADS overrides).  The reference runs one single-threaded process per bucket.
StageSettings StageSettings::from_env() {
  StageSettings s;
  auto num = [](const char *name, long lo, long hi, long dflt) {
    const char *e = getenv(name);
    if (!e || !*e) return dflt;
    char *end = nullptr;
    const long v = strtol(e, &end, 10);
    if (end == e || *end) throw std::string(name) + "=" + e + ": not a number";
    if (v < lo || v > hi) throw std::string(name) + "=" + e + ": out of range";
    return v;
  };
  s.device = (int)num("SDF_DEVICE", 0, 1023, 0);
  s.lanes = (int)num("SDF_LANES", 0, 8, 0);
  s.super_batch = (int)num("SDF_SUPER_BATCH", 0, 1 << 30, 0);
  s.gpu_anchors = num("SDF_GPU_ANCHORS", 0, 1, 1) != 0;
  s.host_threads = (int)num("SDF_HOST_THREADS", 0, 4096, 0);
  if (const char *e = getenv("SDF_STAGE_WS_GIB")) s.stage_ws_gib = atof(e) > 0 ? atof(e) : 0;
  s.debug_timing = getenv("SDF_DEBUG_TIMING") != nullptr;
  s.resident_dp = num("SDF_RESIDENT_DP", 0, 1, 1) != 0;
  s.anchor_parts = (int)num("SDF_ANCHOR_PARTS", 0, 16, 0);
  s.bucket_lanes = (int)num("SDF_BUCKET_LANES", 1, 4, 2);
  s.translate_limit = (int)num("SDF_TEST_TRANSLATE_LIMIT", 1, 0x7fffffff, 100 * 1000 * 1000);
  s.stats_resident = num("SDF_STATS_RESIDENT", 0, 1, 0) != 0;
  s.stats_cuts_device = num("SDF_STATS_CUTS_DEVICE", 0, 1, 0) != 0;
  s.stats_diff_host = num("SDF_STATS_DIFF_HOST", 0, 1, 0) != 0;
  s.search_wide = (int)num("SDF_SEARCH_WIDE_DEVICE", 0, 1 << 20, 0);
  s.search_lanes = (int)num("SDF_SEARCH_LANES", 1, 16, 1);
  s.stage_resident = num("SDF_STAGE_RESIDENT", 0, 1, 0) != 0;
  s.fetch_device = num("SDF_STAGE_FETCH_DEVICE", 0, 1, 0) != 0;
  if (const char *e = getenv("SDF_DEVICES"))
    for (const char *c = e; *c;) {
      char *end = nullptr;
      const long d = strtol(c, &end, 10);
      if (end == c) throw std::string("SDF_DEVICES=") + e + ": a list of device ordinals";
      s.devices.push_back((int)d);
      c = *end == ',' ? end + 1 : end;
    }
  return s;
}
namespace {
StageSettings g_stage_settings;
std::mutex g_stage_settings_mu;
}  // namespace
const StageSettings &stage_settings() { return g_stage_settings; }
void set_stage_settings(const StageSettings &s) {
  std::lock_guard<std::mutex> g(g_stage_settings_mu);
  g_stage_settings = s;
}

namespace {
// The first failure of the threads that work for one caller: recorded in their catch blocks -- whatever was thrown --, rethrown
// on the caller's thread, once they have all returned, as the std::string message the stage's callers handle.
class FirstError {
 public:
  void set() {  // (inside a catch block)
    std::string msg;
    try {
      throw;
    } catch (std::string &s) {
      msg = s.empty() ? std::string("error") : s;
    } catch (std::exception &e) {
      msg = e.what();
    } catch (...) {
      msg = "unknown error";
    }
    std::lock_guard<std::mutex> g(mu_);
    if (!failed_) msg_ = msg;
    failed_ = true;
  }
  bool failed() const { return failed_; }
  void rethrow() const {
    if (failed_) throw msg_;
  }

 private:
  std::mutex mu_;
  std::atomic<bool> failed_{false};
  std::string msg_;
};
}  // namespace

static void parallel_for(int n, const std::function<void(int)> &body) {
  const int nthreads = [] {
    const int asked = stage_settings().host_threads;
    int t = asked > 0 ? asked : (int)std::thread::hardware_concurrency();
    if (asked <= 0) {  // a container's CPU quota (cgroup v2 cpu.max = "<quota> <period>") counts, not the host's core count
      if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
        long long quota = 0, period = 0;
        if (fscanf(f, "%lld %lld", &quota, &period) == 2 && quota > 0 && period > 0)
          t = std::min<long long>(t, std::max<long long>(1, (quota + period - 1) / period));
        fclose(f);
      }
    }
    return t < 1 ? 1 : (t > 64 ? 64 : t);
  }();
  const int nt = std::min(nthreads, n);
  if (nt <= 1) {
    for (int i = 0; i < n; i++) body(i);
    return;
  }
  // The lanes of the stage driver call this concurrently, a few hundred times per run.  One set of worker threads for
  // the whole process (as many as the CPU quota: more runnable threads get the process throttled) serves all callers:
  // a call is a REGION -- a counter over its items -- queued for the workers; the caller works on its own region too,
  // so it never waits for a parked thread to wake up, and returns when all its items are done.  (Threads created and
  // joined per call cost 0.1 ms each, milliseconds under a CPU quota.)
  struct Region {
    const std::function<void(int)> *body;
    int n;
    std::atomic<int> next{0}, done{0};
    FirstError error;
    void run() {
      for (int i = next.fetch_add(1); i < n; i = next.fetch_add(1)) {
        try {
          (*body)(i);
        } catch (...) {
          error.set();
        }
        if (done.fetch_add(1) + 1 == n) {  // the last item: wake the caller if it is waiting
          std::lock_guard<std::mutex> g(fin_mu);
          fin_cv.notify_all();
        }
      }
    }
    std::mutex fin_mu;
    std::condition_variable fin_cv;
  };
  struct Pool {
    std::mutex mu;
    std::condition_variable cv;
    std::deque<std::shared_ptr<Region>> open;  // regions that may still have items to hand out
    std::vector<std::thread> workers;
    bool quit = false;
    explicit Pool(int nw) {
      for (int t = 0; t < nw; t++)
        workers.emplace_back([this] {
          for (;;) {
            std::shared_ptr<Region> r;
            {
              std::unique_lock<std::mutex> g(mu);
              cv.wait(g, [&] {
                while (!open.empty() && open.front()->next.load() >= open.front()->n) open.pop_front();
                return quit || !open.empty();
              });
              if (open.empty()) return;
              r = open.front();  // (to the back: the next worker takes another caller's region -- the lanes share the
              open.pop_front();  // workers instead of queueing behind each other)
              open.push_back(r);
            }
            r->run();
          }
        });
    }
    ~Pool() {
      {
        std::lock_guard<std::mutex> g(mu);
        quit = true;
      }
      cv.notify_all();
      for (auto &t : workers) t.join();
    }
  };
  static Pool pool(nthreads);
  auto region = std::make_shared<Region>();
  region->body = &body;
  region->n = n;
  {
    std::lock_guard<std::mutex> g(pool.mu);
    pool.open.push_back(region);
  }
  pool.cv.notify_all();
  region->run();
  if (region->done.load() < n) {  // (workers still inside their last items: sleep, a spinning caller eats CPU quota)
    std::unique_lock<std::mutex> g(region->fin_mu);
    region->fin_cv.wait(g, [&] { return region->done.load() >= n; });
  }
  region->error.rethrow();
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
using Clock = std::chrono::steady_clock;
double since(Clock::time_point a) { return std::chrono::duration<double>(Clock::now() - a).count(); }

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
    for (int k = 0; k < n; k++) {
      Item &it = items[k];
      it.h = run.schedule[base + k];
      span[2 * k] = run.fr->locate(it.h.query->name, it.h.query_start, &it.h.query_end);
      span[2 * k + 1] = run.fr->locate(it.h.ref->name, it.h.ref_start, &it.h.ref_end);
    }
    char *pool = nullptr;
    size_t bytes = 0;
    auto lay_out = [&](const std::vector<size_t> &need) {  // a slot of need[i] bytes per sequence, in the pool
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
    std::vector<size_t> need(2 * (size_t)n);
    ++a.batches;
    bool fetched = false;
    if (genome && stage_settings().fetch_device) {
      // Resident chromosomes hold these bases already: ONE device call of 2n ranges -- the query forward, the reference
      // reverse-complemented on its way where the hit says so -- writes them into slots as long as the bases (locate() has
      // clamped the ends).  A call that fails is said in one line, and this super-batch cuts its sequences out of the file.
      std::vector<int64_t> off(2 * (size_t)n);
      std::vector<int32_t> len(2 * (size_t)n);
      std::vector<char> rc(2 * (size_t)n, 0);
      std::string why;
      for (int k = 0; k < n && why.empty(); k++) {
        const Hit &h = items[k].h;
        int64_t qb = 0, rb = 0;
        if (!dp.chromosome_base(h.query->name, &qb) || !dp.chromosome_base(h.ref->name, &rb)) {
          why = "a pair on a chromosome that is not resident";
          break;
        }
        off[2 * k] = qb + std::max(0, h.query_start);
        off[2 * k + 1] = rb + std::max(0, h.ref_start);
        len[2 * k] = span[2 * k].bytes ? std::max(0, h.query_end - std::max(0, h.query_start)) : 0;
        len[2 * k + 1] = span[2 * k + 1].bytes ? std::max(0, h.ref_end - std::max(0, h.ref_start)) : 0;
        rc[2 * k + 1] = h.ref->is_rc;
        need[2 * k] = (size_t)len[2 * k], need[2 * k + 1] = (size_t)len[2 * k + 1];
      }
      if (why.empty()) {
        lay_out(need);
        fetched = dp.fetch_ranges(off.data(), len.data(), rc.data(), slot.data(), off.size(), pool, bytes, why);
      }
      if (fetched) {
        ++a.fetched_device;
        parallel_for(n, [&](int k) {
          Item &it = items[k];
          it.fa = SeqView(pool + slot[2 * k], need[2 * k]);
          it.fb = SeqView(pool + slot[2 * k + 1], need[2 * k + 1]);
          it.job.reset(new PairJob(it.fa, it.fb, it.h, run.p, !genome));
        });
      } else {
        fprintf(stderr, "[sedef_amd] SDF_STAGE_FETCH_DEVICE=1: super-batch at pair %d cuts its sequences out of the FASTA file: %s\n",
                base, why.c_str());
      }
    }
    if (!fetched) {
      for (size_t i = 0; i < 2 * (size_t)n; i++) need[i] = span[i].bytes;
      lay_out(need);
      parallel_for(n, [&](int k) {
        Item &it = items[k];
        char *qa = pool + slot[2 * k], *ra = pool + slot[2 * k + 1];
        it.fa = SeqView(qa, FastaReference::extract(span[2 * k], qa));
        it.fb = SeqView(ra, FastaReference::extract(span[2 * k + 1], ra));
        if (it.h.ref->is_rc) rc_inplace(ra, it.fb.size());
        it.job.reset(new PairJob(it.fa, it.fb, it.h, run.p, !genome));
      });
    }
    ++g_totals.batches;
    if (genome) {
      // Nothing is uploaded: the pairs' ranges of the resident chromosomes, and ONE device call that says which pairs hold
      // nothing but ACGTNacgtn (PairJob's own scan of every character otherwise).
      std::vector<int64_t> off(2 * (size_t)n);
      std::vector<int32_t> len(2 * (size_t)n);
      std::vector<char> plain(2 * (size_t)n);
      for (int k = 0; k < n; k++) {
        const Hit &h = items[k].h;
        int64_t qb = 0, rb = 0;
        if (!dp.chromosome_base(h.query->name, &qb) || !dp.chromosome_base(h.ref->name, &rb))
          throw std::string("internal: a pair on a chromosome that is not resident");
        off[2 * k] = q_base[k] = qb + std::max(0, h.query_start);
        off[2 * k + 1] = r_base[k] = rb + std::max(0, h.ref_start);
        len[2 * k] = (int32_t)items[k].fa.size();
        len[2 * k + 1] = (int32_t)items[k].fb.size();
      }
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

// body(0) on the calling thread, body(1 .. n - 1) on threads of their own, until all have returned; the first failure of any
// of them is left in `failure` (which tells the others that one has failed) for the caller to rethrow.
void run_lanes(int n, FirstError &failure, const std::function<void(int)> &body) {
  auto one = [&](int l) {
    try {
      body(l);
    } catch (...) {
      failure.set();
    }
  };
  std::vector<std::thread> threads;
  for (int l = 1; l < n; l++) threads.emplace_back(one, l);
  one(0);
  for (auto &t : threads) t.join();
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
      while (std::getline(fin, line)) {
        size_t at = 0;
        for (int col = 0; col < 4 && at <= line.size(); col++) {
          const size_t e = std::min(line.find('\t', at), line.size());
          if ((col == 0 || col == 3) && e > at && seen.insert(line.substr(at, e - at)).second) names.push_back(line.substr(at, e - at));
          at = e + 1;
        }
      }
    }
    const auto t0 = std::chrono::steady_clock::now();
    FastaReference fr(ref_path);
    ok = dp.load_genome(fr, names, max_batch_bytes, why);
    if (ok && st.debug_timing)
      fprintf(log, "[resident chromosomes: %zu records loaded and shared in %.1f ms]\n", names.size(),
              std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
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
