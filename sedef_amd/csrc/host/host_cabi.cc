// C ABI of the host pipeline (used by the CLI wrapper tests and by the Python tests through ctypes).
// `test_dp` arguments are TEST HOOKS: a non-NULL function with the oracle's single-task signature
// replaces the GPU provider; the CLI always passes NULL.
#include <cstdio>
#include <cstring>
#include <string>

#include "stage_internal.h"

using namespace sdfh;

static thread_local std::string g_err;

static std::unique_ptr<DpProvider> provider(test_dp_fn fn, int device) {
  set_stage_settings(StageSettings::from_env());  // (every run of an entry point: the stage driver's settings, read here once)
  if (fn) return make_test_provider(fn);
  return make_gpu_provider(device);
}

static int copy_out(const std::string &s, char *buf, size_t cap) {
  if (s.size() + 1 > cap) {
    g_err = "output buffer too small";
    return -2;
  }
  memcpy(buf, s.c_str(), s.size() + 1);
  return 0;
}

extern "C" {

const char *sdfh_last_error(void) { return g_err.c_str(); }

// `sedef align generate -k K genome.fa bucket.bed > out` (reference: src/align_main.cc:285-337)
int sdfh_generate(const char *ref_path, const char *bed_path, int kmer, const char *out_path, int match,
                  int mismatch, int gap_open, int gap_extend, test_dp_fn test_dp, int device, long long *stats) {
  try {
    Params p;
    p.match = match;
    p.mismatch = mismatch;
    p.gap_open = gap_open;
    p.gap_extend = gap_extend;
    auto dp = provider(test_dp, device);
    FILE *out = out_path ? fopen(out_path, "w") : stdout;
    if (!out) throw std::string("Cannot open output ") + out_path;
    GenerateStats st = generate_alignments(ref_path, bed_path, kmer, p, *dp, out, stderr);
    if (out_path) fclose(out);
    if (stats) {
      stats[0] = st.lines;
      stats[1] = st.total_written;
      stats[2] = st.dp_tasks;
      stats[3] = st.dp_cells;
      stats[4] = st.rounds;
    }
    return 0;
  } catch (std::string &s) {
    g_err = s;
    return -1;
  } catch (std::exception &e) {
    g_err = e.what();
    return -1;
  }
}

// several buckets, one provider (host/stage_driver.cc: generate_many): `beds` = bucket paths separated by newlines; every
// bucket's lines go to `<bucket><out_suffix>`.  stats: per bucket {lines, hits} (2 x buckets entries).
// `totals`: behind them the four totals of the process (stage_totals).  resident: StageSettings::stage_resident for this
// run -- the lanes' providers are then set up side by side, as the CLI does, and the chromosomes loaded before the stage.
static int generate_many_impl(const char *ref_path, const char *beds, int kmer, const char *out_suffix, const char *log_dir,
                              test_dp_fn test_dp, int device, bool resident, bool totals, long long *stats) {
  try {
    Params p;
    std::vector<std::string> list;
    for (const char *c = beds; *c;) {
      const char *e = strchr(c, '\n');
      std::string one = e ? std::string(c, e) : std::string(c);
      if (!one.empty()) list.push_back(one);
      if (!e) break;
      c = e + 1;
    }
    const std::vector<std::string> buckets = expand_buckets(list);
    std::unique_ptr<DpProvider> dp;
    stage_totals_reset();
    if (resident && !test_dp) {  // (the CPU path keeps no chromosomes anywhere: the hook ignores the mode)
      StageSettings s = StageSettings::from_env();
      s.stage_resident = true;
      set_stage_settings(s);
      const StageHint hint = stage_hint_many(buckets);
      dp = make_gpu_providers(device, hint.lanes, hint.devices, hint.max_batch_bytes);
      load_stage_genome(*dp, ref_path, buckets, kmer, hint.max_batch_bytes, stderr);
    } else {
      dp = provider(test_dp, device);
      if (!test_dp) load_stage_genome(*dp, ref_path, buckets, kmer, stage_hint_many(buckets).max_batch_bytes, stderr);
    }
    const auto sts = generate_many(ref_path, buckets, kmer, p, *dp, out_suffix, log_dir ? log_dir : "", stderr);
    for (size_t k = 0; stats && k < sts.size(); k++) stats[2 * k] = sts[k].lines, stats[2 * k + 1] = sts[k].total_written;
    if (stats && totals) stage_totals(stats + 2 * sts.size());
    return (int)sts.size();
  } catch (std::string &s) {
    g_err = s;
    return -1;
  } catch (std::exception &e) {
    g_err = e.what();
    return -1;
  }
}
int sdfh_generate_many(const char *ref_path, const char *beds, int kmer, const char *out_suffix, const char *log_dir,
                       test_dp_fn test_dp, int device, long long *stats) {
  return generate_many_impl(ref_path, beds, kmer, out_suffix, log_dir, test_dp, device, false, false, stats);
}
// ... on chromosomes that stay resident in HBM (resident != 0, or SDF_STAGE_RESIDENT=1 in the environment; resident == 0
// without the variable: sdfh_generate_many).  stats: 2 x buckets entries, then FASTA records uploaded, characters uploaded
// to a device pool, super-batches run, super-batches that named resident ranges.
int sdfh_generate_many_resident(const char *ref_path, const char *beds, int kmer, const char *out_suffix, const char *log_dir,
                                test_dp_fn test_dp, int device, int resident, long long *stats) {
  return generate_many_impl(ref_path, beds, kmer, out_suffix, log_dir, test_dp, device,
                            resident != 0 || StageSettings::from_env().stage_resident, true, stats);
}
// resident_range (host/stage_driver.cc; test hook): 0 and *off, or -1 when the request is not inside the host's copy
int sdfh_resident_range(long long base, long long start, long long seq_len, long long s, long long len, int rc, long long *off) {
  int64_t o = 0;
  if (!resident_range(base, start, seq_len, s, len, rc != 0, &o)) return -1;
  *off = o;
  return 0;
}
// the DP tasks a request of qlen x tlen bases is cut into, `step` bases at a time (host/dp_provider.cc: for_each_chunk; test
// hook): per chunk {first query base, first byte of the target in pool order -- of a target that starts at t_off and, with t_rc,
// is read reversed --, query length, target length} into out[0, 4 * cap); returns the number of chunks, or -1
long sdfh_dp_chunks(int qlen, int tlen, int step, int t_rc, long long t_off, long long *out, long cap) {
  if (qlen < 0 || tlen < 0 || step < 1 || cap < 0) return -1;
  return (long)dp_chunks(qlen, tlen, (size_t)step, t_rc != 0, t_off, out, (size_t)cap);
}

// `sedef stats generate genome.fa final.bed > out` (reference: src/stats_main.cc:339-389); test_cols: the oracle's column
// walker instead of the device (CPU tests).  stats: hits read, pieces, columns; returns the lines written or -1.
// resident != 0, or SDF_STATS_RESIDENT=1 in the environment: StatsParams::resident.
static long stats_generate_impl(const char *ref_path, const char *bed_path, const char *out_path, int max_ok_gap, int min_split,
                                int min_uppercase, double max_error, test_cols_fn test_cols, test_cuts_fn test_cuts, int device,
                                int resident, int cuts, long long *stats) {
  try {
    StatsParams sp;
    sp.resident = resident != 0 || StageSettings::from_env().stats_resident;
    sp.cuts_device = cuts != 0;
    sp.max_ok_gap = max_ok_gap;
    sp.min_split = min_split;
    sp.min_uppercase = min_uppercase;
    sp.max_scaled_error = max_error;
    struct Out {  // (closed on every path; a run that throws leaves no truncated table behind -- ADVICE r3)
      FILE *f = nullptr;
      std::string path;
      bool done = false;
      ~Out() {
        if (f) fclose(f);
        if (f && !done) remove(path.c_str());
      }
    } out;
    out.path = out_path;
    out.f = fopen(out_path, "w");
    if (!out.f) throw std::string("Cannot open output ") + out_path;
    const long lines = stats_generate(ref_path, bed_path, out.f, sp, test_cols, device, stats, test_cuts);
    out.done = true;
    return lines;
  } catch (std::string &s) {
    g_err = s;
    return -1;
  } catch (std::exception &e) {
    g_err = e.what();
    return -1;
  }
}

long sdfh_stats_generate_resident(const char *ref_path, const char *bed_path, const char *out_path, int max_ok_gap, int min_split,
                                  int min_uppercase, double max_error, test_cols_fn test_cols, int device, int resident,
                                  long long *stats) {
  return stats_generate_impl(ref_path, bed_path, out_path, max_ok_gap, min_split, min_uppercase, max_error, test_cols, nullptr, device,
                             resident, 0, stats);
}

// ... with the cuts and trims on the device too (cuts != 0, or SDF_STATS_CUTS_DEVICE=1 in the environment:
// StatsParams::cuts_device; only together with resident chromosomes and without max_ok_gap).  test_cuts: a CPU stand-in for
// sdf_stats_cuts_pairs (sedef_host.h: test_cuts_fn) -- the new host path then runs without a device, with test_cols for the columns.
long sdfh_stats_generate_cuts(const char *ref_path, const char *bed_path, const char *out_path, int max_ok_gap, int min_split,
                              int min_uppercase, double max_error, test_cols_fn test_cols, int device, int resident, int cuts,
                              test_cuts_fn test_cuts, long long *stats) {
  return stats_generate_impl(ref_path, bed_path, out_path, max_ok_gap, min_split, min_uppercase, max_error, test_cols, test_cuts,
                             device, resident, cuts != 0 || StageSettings::from_env().stats_cuts_device, stats);
}

long sdfh_stats_generate(const char *ref_path, const char *bed_path, const char *out_path, int max_ok_gap, int min_split,
                         int min_uppercase, double max_error, test_cols_fn test_cols, int device, long long *stats) {
  return sdfh_stats_generate_resident(ref_path, bed_path, out_path, max_ok_gap, min_split, min_uppercase, max_error, test_cols,
                                      device, 0, stats);
}

// stats_piece_range (host/stats.cc; test hook): returns the length, *first the chromosome's first base of the range
int sdfh_stats_piece_range(int start, int end, int s, int e, int rc, long long *first) {
  return stats_piece_range(start, end, s, e, rc != 0, first);
}

// fmt 4.0.1 "{}" of a double, as `stats generate` prints it (test hook)
int sdfh_format_double(double x, char *buf, size_t cap) { return copy_out(format_double(x), buf, cap); }

// Alignment(fa, fb) (reference: src/align.cc:76-88): CIGAR string + counters {matches, mismatches, gaps, gap_bases, span}
static int alignment_pair_impl(const Params &p, const char *fa, const char *fb, test_dp_fn test_dp, int device,
                               char *cigar, size_t cap, int *counts);
int sdfh_alignment_pair(const char *fa, const char *fb, test_dp_fn test_dp, int device, char *cigar, size_t cap,
                        int *counts) {
  return alignment_pair_impl(Params(), fa, fb, test_dp, device, cigar, cap, counts);
}
// the same with the CLI's scoring overrides (reference: src/align_main.cc:343-352)
int sdfh_alignment_pair_scored(const char *fa, const char *fb, int match, int mismatch, int gap_open, int gap_extend,
                               test_dp_fn test_dp, int device, char *cigar, size_t cap, int *counts) {
  Params p;
  p.match = match;
  p.mismatch = mismatch;
  p.gap_open = gap_open;
  p.gap_extend = gap_extend;
  const int rc = alignment_pair_impl(p, fa, fb, test_dp, device, cigar, cap, counts);
  set_alignment_scoring(Params());
  return rc;
}
static int alignment_pair_impl(const Params &p, const char *fa, const char *fb, test_dp_fn test_dp, int device,
                               char *cigar, size_t cap, int *counts) {
  try {
    set_alignment_scoring(p);
    auto dp = provider(test_dp, device);
    const std::string sa = fa, sb = fb;  // (requests point into the sequences: they live until the DP has run)
    std::vector<DpRequest> reqs;
    DpSession rec;
    rec.requests = &reqs;
    { Alignment tmp(sa, sb, rec); }
    std::vector<Cigar> res = dp->run_cigars(reqs, p);
    DpSession rep;
    rep.recording = false;
    rep.results = &res;
    Alignment al(sa, sb, rep);
    counts[0] = al.matches();
    counts[1] = al.mismatches();
    counts[2] = al.gaps();
    counts[3] = al.gap_bases();
    counts[4] = al.span();
    return copy_out(al.cigar_string(), cigar, cap);
  } catch (std::string &s) {
    g_err = s;
    return -1;
  }
}

// Guide alignment of refined chains (reference: src/align.cc:107-197 after optional merges, src/refine.cc:165-183).
// Hits are given as coordinates + CIGAR strings over qstr/rstr; consecutive overlapping hits are merged
// like refine_chains does.  Output: "qs qe rs re cigar matches mismatches gaps gap_bases".
int sdfh_guide_alignment(const char *qstr_, const char *rstr_, int n, const int *coords, const char **cigars, int side,
                         test_dp_fn test_dp, int device, char *outbuf, size_t cap) {
  try {
    Params p;
    set_alignment_scoring(p);
    auto dp = provider(test_dp, device);
    const std::string qstr = qstr_, rstr = rstr_;
    auto qs = std::make_shared<Sequence>("QRY", qstr);
    auto rs = std::make_shared<Sequence>("REF", rstr);
    std::vector<Hit> hits(n);
    for (int k = 0; k < n; k++) {
      Hit &h = hits[k];
      h.query = qs;
      h.ref = rs;
      h.query_start = coords[4 * k];
      h.query_end = coords[4 * k + 1];
      h.ref_start = coords[4 * k + 2];
      h.ref_end = coords[4 * k + 3];
      h.aln = Alignment(qstr.substr(h.query_start, h.query_end - h.query_start),
                        rstr.substr(h.ref_start, h.ref_end - h.ref_start), std::string(cigars[k]));
      h.aln.start_a = h.query_start;
      h.aln.end_a = h.query_end;
      h.aln.start_b = h.ref_start;
      h.aln.end_b = h.ref_end;
    }
    auto with_dp = [&](std::function<void(DpSession &)> body_rec, std::function<void(DpSession &)> body_real) {
      std::vector<DpRequest> reqs;
      DpSession rec;
      rec.requests = &reqs;
      body_rec(rec);
      std::vector<Cigar> res = dp->run_cigars(reqs, p);
      DpSession rep;
      rep.recording = false;
      rep.results = &res;
      body_real(rep);
    };
    std::vector<Hit> guide;
    Hit *prev = &hits[0];
    for (int pi = 1; pi < n; pi++) {
      Hit &cur = hits[pi];
      if (cur.query_start < prev->query_end || cur.ref_start < prev->ref_end) {
        with_dp([&](DpSession &d) { Alignment a = prev->aln, c = cur.aln; a.merge(c, qstr, rstr, d); },
                [&](DpSession &d) { prev->aln.merge(cur.aln, qstr, rstr, d); });
        update_from_alignment(*prev);
      } else {
        guide.push_back(*prev);
        prev = &cur;
      }
    }
    guide.push_back(*prev);
    Alignment fin;
    with_dp([&](DpSession &d) { Alignment t(qstr, rstr, guide, side, d); },
            [&](DpSession &d) { fin = Alignment(qstr, rstr, guide, side, d); });
    char head[256];
    snprintf(head, sizeof head, "%d %d %d %d ", fin.start_a, fin.end_a, fin.start_b, fin.end_b);
    char tail[128];
    snprintf(tail, sizeof tail, " %d %d %d %d", fin.matches(), fin.mismatches(), fin.gaps(), fin.gap_bases());
    return copy_out(std::string(head) + fin.cigar_string() + tail, outbuf, cap);
  } catch (std::string &s) {
    g_err = s;
    return -1;
  }
}

// Chains given as anchor lists "q,r,l;q,r,l|q,r,l;...": builds every chain alignment (src/align.cc:199-270),
// merges overlapping neighbours and builds the guide alignment with side extension, like refine_chains does for
// one path (src/refine.cc:163-183).  Output: "qs qe rs re cigar matches mismatches gaps gap_bases|to_bed line".
int sdfh_guide_from_chains(const char *qstr_, const char *rstr_, const char *spec, int side, test_dp_fn test_dp,
                           int device, char *outbuf, size_t cap) {
  try {
    Params p;
    set_alignment_scoring(p);
    auto dp = provider(test_dp, device);
    const std::string qstr = qstr_, rstr = rstr_;
    std::vector<std::vector<Anchor>> chains(1);
    for (const char *c = spec; *c;) {
      if (*c == '|') {
        chains.push_back({});
        c++;
        continue;
      }
      int q, r, l, n = 0;
      if (sscanf(c, "%d,%d,%d%n", &q, &r, &l, &n) != 3) break;
      chains.back().push_back(Anchor{q, r, l, 0});
      c += n;
      if (*c == ';') c++;
    }
    if (chains.back().empty()) chains.pop_back();
    auto with_dp = [&](std::function<void(DpSession &)> body) {
      std::vector<DpRequest> reqs;
      DpSession rec;
      rec.requests = &reqs;
      body(rec);  // recording pass (callers pass bodies that work on copies)
      return dp->run_cigars(reqs, p);
    };
    auto qs = std::make_shared<Sequence>("QRY", qstr);
    auto rs = std::make_shared<Sequence>("REF", rstr);
    std::vector<Hit> hits(chains.size());
    for (size_t k = 0; k < chains.size(); k++) {
      std::vector<int> idx;
      for (int i = 0; i < (int)chains[k].size(); i++) idx.push_back(i);
      auto res = with_dp([&](DpSession &d) { Alignment t(qstr, rstr, chains[k], idx, d); });
      DpSession rep;
      rep.recording = false;
      rep.results = &res;
      hits[k].query = qs;
      hits[k].ref = rs;
      hits[k].aln = Alignment(qstr, rstr, chains[k], idx, rep);
      update_from_alignment(hits[k]);
    }
    std::vector<Hit> guide;
    Hit *prev = &hits[0];
    for (size_t pi = 1; pi < hits.size(); pi++) {
      Hit &cur = hits[pi];
      if (cur.query_start < prev->query_end || cur.ref_start < prev->ref_end) {
        auto res = with_dp([&](DpSession &d) { Alignment a = prev->aln, c = cur.aln; a.merge(c, qstr, rstr, d); });
        DpSession rep;
        rep.recording = false;
        rep.results = &res;
        prev->aln.merge(cur.aln, qstr, rstr, rep);
        update_from_alignment(*prev);
      } else {
        guide.push_back(*prev);
        prev = &cur;
      }
    }
    guide.push_back(*prev);
    auto res = with_dp([&](DpSession &d) { Alignment t(qstr, rstr, guide, side, d); });
    DpSession rep;
    rep.recording = false;
    rep.results = &res;
    Hit fin;
    fin.query = qs;
    fin.ref = rs;
    fin.name = "name";
    fin.comment = "cmt";
    fin.aln = Alignment(qstr, rstr, guide, side, rep);
    update_from_alignment(fin);
    char head[256], tail[128];
    snprintf(head, sizeof head, "%d %d %d %d ", fin.query_start, fin.query_end, fin.ref_start, fin.ref_end);
    snprintf(tail, sizeof tail, " %d %d %d %d|", fin.aln.matches(), fin.aln.mismatches(), fin.aln.gaps(),
             fin.aln.gap_bases());
    return copy_out(std::string(head) + fin.aln.cigar_string() + tail + fin.to_bed(false), outbuf, cap);
  } catch (std::string &s) {
    g_err = s;
    return -1;
  }
}

// fast_align(query, ref, orig, kmer) (reference: src/chain.cc:203-268, the per-pair entry src/align_main.cc:313 and
// python/sedef.cpp:85 call): seed anchors, chains, chain alignments, refine_chains.  `orig` is given by the fields the
// path reads: the two names and strands (same-chromosome rules, src/chain.cc:45-46, src/refine.cc:29-30) and the two
// start coordinates.  Output: one line per refined hit, coordinates relative to the two strings:
// "qs qe rs re cigar matches mismatches gaps gap_bases\n".
int sdfh_fast_align(const char *query_, const char *ref_, const char *qname, const char *rname, int q_rc, int r_rc,
                    int qstart, int rstart, int kmer, test_dp_fn test_dp, int device, char *outbuf, size_t cap) {
  try {
    Params p;
    p.kmer = kmer;
    set_alignment_scoring(p);
    auto dp = provider(test_dp, device);
    const std::string query = query_, ref = ref_;
    Hit orig;
    orig.query = std::make_shared<Sequence>(qname, "", false);
    orig.ref = std::make_shared<Sequence>(rname, "", false);
    orig.query->is_rc = q_rc != 0;
    orig.ref->is_rc = r_rc != 0;
    orig.query_start = qstart;
    orig.ref_start = rstart;
    orig.query_end = qstart + (int)query.size();
    orig.ref_end = rstart + (int)ref.size();
    PairJob job(query, ref, orig, p);
    std::vector<Cigar> results;
    for (;;) {
      std::vector<DpRequest> reqs = job.advance(results);
      if (reqs.empty()) break;
      results = dp->run_cigars(reqs, p);
    }
    std::string out;
    char nums[160];
    for (auto &h : job.hits()) {
      snprintf(nums, sizeof nums, "%d %d %d %d ", h.query_start, h.query_end, h.ref_start, h.ref_end);
      out += nums;
      out += h.aln.cigar_string();
      snprintf(nums, sizeof nums, " %d %d %d %d\n", h.aln.matches(), h.aln.mismatches(), h.aln.gaps(), h.aln.gap_bases());
      out += nums;
    }
    return copy_out(out, outbuf, cap);
  } catch (std::string &s) {
    g_err = s;
    return -1;
  } catch (std::exception &e) {
    g_err = e.what();
    return -1;
  }
}

// FastaReference::get_sequence (reference: src/fasta.cc:105-142); *end is updated like the reference does
int sdfh_fasta_get(const char *path, const char *name, int start, int *end, char *buf, size_t cap) {
  try {
    FastaReference fr(path);
    std::string s = fr.get_sequence(name, start, end);
    return copy_out(s, buf, cap);
  } catch (std::string &s) {
    g_err = s;
    return -1;
  }
}

// merge() of src/merge.cc:35-109 on BED lines (one per line in `lines`); output: merged BED lines
int sdfh_merge(const char *lines, int merge_dist, char *buf, size_t cap) {
  try {
    std::vector<Hit> hits;
    for (auto &l : split(lines, '\n'))
      if (!l.empty()) hits.push_back(Hit::from_bed(l));
    auto res = merge_hits(hits, merge_dist);
    std::string out;
    for (auto &h : res) out += h.to_bed(false) + "\n";
    return copy_out(out, buf, cap);
  } catch (std::string &s) {
    g_err = s;
    return -1;
  }
}

// `sedef align bucket -n N bed_path out_dir genome.fa` (reference: src/align_main.cc:38-198)
int sdfh_bucket(const char *bed_path, int nbins, const char *out_dir, const char *reference) {
  try {
    BucketParams bp;
    bucket_alignments_extern(bed_path, nbins, out_dir, true, reference, bp, stderr);
    return 0;
  } catch (std::string &s) {
    g_err = s;
    return -1;
  }
}

// ... through the records of include/sedef_hip.h (bucket_alignments_records) -- form 1: sdf_bucket_merge on `device`, form 2:
// sdf_bucket_merge_host.  Returns 1 when the bucket files were written, 0 when the seeds keep the host path (nothing written).
int sdfh_bucket_records(const char *bed_path, int nbins, const char *out_dir, const char *reference, int form, int device) {
  try {
    BucketParams bp;
    return bucket_alignments_records(bed_path, nbins, out_dir, reference, bp, stderr, form, device) ? 1 : 0;
  } catch (std::string &s) {
    g_err = s;
    return -1;
  }
}

// `sedef stats recall final.bed wgac.tab out.txt` (stats_recall.cc): the MISS and PART lines to out_path, the four summary lines
// of the command's stdout to buf.  host != 0: sdf_pair_recall_host, no device.
int sdfh_stats_recall(const char *bed_path, const char *wgac_path, const char *out_path, int host, int ignore_strand, int device, char *buf,
                      size_t cap) {
  char *text = nullptr;
  size_t len = 0;
  FILE *report = open_memstream(&text, &len);
  if (!report) {
    g_err = "open_memstream failed";
    return -1;
  }
  int rc = 0;
  try {
    stats_recall(bed_path, wgac_path, out_path, host != 0, ignore_strand != 0, device, report, stderr);
  } catch (std::string &s) {
    g_err = s;
    rc = -1;
  }
  fclose(report);
  if (rc == 0) rc = copy_out(std::string(text, len), buf, cap);
  free(text);
  return rc;
}

// `sedef report genome.fa inputs... out_dir` (report_cmd.cc): `inputs` is a newline-separated list of *.aligned.bed files or
// directories of them; counts: the lines of out_dir/aligned.bed and out_dir/final.bed.  host != 0, or SDF_REPORT_HOST=1 in the
// environment: the two orderings by sdf_line_order_host.  The stats parameters and SDF_STATS_RESIDENT / SDF_STATS_CUTS_DEVICE as
// for sdfh_stats_generate_cuts.
int sdfh_report(const char *ref_path, const char *inputs, const char *out_dir, int max_ok_gap, int min_split, int min_uppercase,
                double max_error, int host, int device, long long *counts) {
  try {
    const StageSettings env = StageSettings::from_env();
    StatsParams sp;
    sp.resident = env.stats_resident;
    sp.cuts_device = env.stats_cuts_device;
    sp.max_ok_gap = max_ok_gap;
    sp.min_split = min_split;
    sp.min_uppercase = min_uppercase;
    sp.max_scaled_error = max_error;
    return report_command(ref_path, split(inputs, '\n'), out_dir, sp, host != 0 || env.report_host, device, stderr, counts);
  } catch (std::string &s) {
    g_err = s;
    return -1;
  } catch (std::exception &e) {
    g_err = e.what();
    return -1;
  }
}

// generate_anchors on the host (reference: src/chain.cc:24-101): "q r l has_u;" per anchor, in order
int sdfh_anchors(const char *query, const char *ref, int kmer, int same_chr, int qstart, int rstart, char *buf,
                 size_t cap) {
  try {
    Hit orig;
    orig.query = std::make_shared<Sequence>("A", "");
    orig.ref = std::make_shared<Sequence>(same_chr ? "A" : "B", "");
    orig.query_start = qstart;
    orig.ref_start = rstart;
    std::vector<Anchor> an = generate_anchors(query, ref, orig, kmer);
    std::string out;
    char t[96];
    for (auto &a : an) {
      snprintf(t, sizeof t, "%d %d %d %d;", a.q, a.r, a.l, a.has_u);
      out += t;
    }
    return copy_out(out, buf, cap);
  } catch (std::string &s) {
    g_err = s;
    return -1;
  }
}

// Chain extraction for one pair: anchors + chains (reference: src/chain.cc:24-199).  Writes
// "q r l has_u" per anchor of each kept chain, chains separated by "|" -- for self-consistency tests.
int sdfh_chains(const char *query, const char *ref, int kmer, char *buf, size_t cap) {
  try {
    Params p;
    p.kmer = kmer;
    Hit orig;
    orig.query = std::make_shared<Sequence>("A", "");
    orig.ref = std::make_shared<Sequence>("B", "");
    std::vector<Anchor> an = generate_anchors(query, ref, orig, kmer);
    auto ch = chain_anchors(an, p);
    std::string out;
    for (size_t bi = 1; bi < ch.second.size(); bi++) {
      for (int k = ch.second[bi].first - 1; k >= ch.second[bi - 1].first; k--) {
        const Anchor &a = an[ch.first[k]];
        char t[96];
        snprintf(t, sizeof t, "%d %d %d %d;", a.q, a.r, a.l, a.has_u);
        out += t;
      }
      out += "|";
    }
    return copy_out(out, buf, cap);
  } catch (std::string &s) {
    g_err = s;
    return -1;
  }
}

// chain_anchors on a caller-provided anchor list: path (m entries), bounds (2*(m+1)), returns #boundaries
int sdfh_chain_raw(const int32_t *anchors, int m, int max_chain_gap, int match_chain_score, int32_t *path,
                   int32_t *bounds) {
  try {
    Params p;
    p.max_chain_gap = max_chain_gap;
    p.match_chain_score = match_chain_score;
    std::vector<Anchor> an(m);
    for (int i = 0; i < m; i++) an[i] = Anchor{anchors[4 * i], anchors[4 * i + 1], anchors[4 * i + 2], anchors[4 * i + 3]};
    auto ch = chain_anchors(an, p);
    for (size_t k = 0; k < ch.first.size(); k++) path[k] = ch.first[k];
    for (size_t b = 0; b < ch.second.size(); b++) {
      bounds[2 * b] = ch.second[b].first;
      bounds[2 * b + 1] = ch.second[b].second ? 1 : 0;
    }
    return (int)ch.second.size();
  } catch (std::string &s) {
    g_err = s;
    return -1;
  }
}

// Test hook: the priority search tree of chain_anchors driven by a script (see chain.cc: rangemax_script)
int sdfh_rangemax_script(const int *pts, int n, const int *ops, int nops, int *out, int *state, int state_cap) {
  return rangemax_script(pts, n, ops, nops, out, state, state_cap);
}

// Hit::extend (reference: src/hit.cc:200-207): io = {query_start, query_end, ref_start, ref_end}
int sdfh_hit_extend(int *io, double factor, int max_extend) {
  Hit h;
  h.query_start = io[0];
  h.query_end = io[1];
  h.ref_start = io[2];
  h.ref_end = io[3];
  h.extend(factor, max_extend);
  io[0] = h.query_start;
  io[1] = h.query_end;
  io[2] = h.ref_start;
  io[3] = h.ref_end;
  return 0;
}

// Sequence ctor (reference: src/hash.cc:104-109): "name|seq|is_rc"
int sdfh_sequence(const char *name, const char *seq, int is_rc, char *buf, size_t cap) {
  Sequence s(name, seq, is_rc != 0);
  return copy_out(s.name + "|" + s.seq + "|" + (s.is_rc ? "1" : "0"), buf, cap);
}

// ---- `sedef search` (search_cmd.cc) ----
// the BED line of a search hit; ref_len: the reference record's length (read under ref_rc alone)
int sdfh_search_hit_bed(const char *qname, const char *rname, int qs, int qe, int rs, int re, int ref_rc, long long ref_len, char *buf,
                        size_t cap) {
  return copy_out(search_hit_bed(qname, rname, qs, qe, rs, re, ref_rc != 0, (size_t)ref_len), buf, cap);
}

// limit[1 .. n] of (k, max_error, max_edit_error) into out[0, n): walk != 0 by the loop as the reference writes it
int sdfh_limit_table(int kmer, double max_error, double max_edit_error, int n, int walk, int *out) {
  for (int s = 1; s <= n; s++)
    out[s - 1] = walk ? relaxed_jaccard_estimate_walk(s, kmer, max_error, max_edit_error) : relaxed_jaccard_estimate(s, kmer, max_error, max_edit_error);
  return 0;
}

// --limit-table parsing: the entries (limit[0] = 0 first) into out[0, cap); returns their number, or -1 with the refusal
int sdfh_read_limit_table(const char *path, int *out, int cap) {
  try {
    const std::vector<int32_t> t = read_limit_table(path);
    for (size_t i = 0; i < t.size() && (int)i < cap; i++) out[i] = t[i];
    return (int)t.size();
  } catch (std::string &s) {
    g_err = s;
    return -1;
  }
}

// the groups of `-t` over the records of genome.fa.fai at a group limit: "name, name|name|..." (groups separated by '|')
int sdfh_translation(const char *ref_path, int max_size, char *buf, size_t cap) {
  try {
    std::string out;
    for (auto &g : generate_translation(ref_path, max_size)) {
      if (!out.empty()) out += "|";
      for (size_t i = 0; i < g.size(); i++) out += (i ? "," : "") + g[i];
    }
    return copy_out(out, buf, cap);
  } catch (std::string &s) {
    g_err = s;
    return -1;
  }
}

// the arguments behind `sedef search`, separated by newlines -> "k w u e E g min_read_size transform reverse|limit table|pos..."
int sdfh_search_args(const char *args, char *buf, size_t cap) {
  try {
    std::vector<std::string> a = split(args, '\n');
    std::vector<char *> argv;
    for (auto &s : a) argv.push_back(&s[0]);
    const SearchParams p = parse_search_args((int)argv.size(), argv.data());
    char head[256];
    snprintf(head, sizeof head, "%d %d %d %.17g %.17g %.17g %d %d %d", p.kmer_size, p.window_size, p.min_uppercase, p.max_error, p.max_edit_error,
             p.gap_frequency, p.min_read_size, (int)p.transform, (int)p.reverse);
    std::string out = std::string(head) + "|" + p.limit_table;
    for (auto &s : p.pos) out += "|" + s;
    return copy_out(out, buf, cap);
  } catch (std::string &s) {
    g_err = s;
    return -1;
  }
}

// ---- `sedef seeds` (seeds_cmd.cc) ----
// the pairs of a run over genome.fa.fai at a group limit, in order: "i j reverse q r same_genome" per pair, separated by '|'
int sdfh_seeds_pairs(const char *ref_path, int max_size, char *buf, size_t cap) {
  try {
    std::string out;
    for (auto &p : seeds_pairs(generate_translation(ref_path, max_size)))
      out += (out.empty() ? "" : "|") + std::to_string(p.i) + " " + std::to_string(p.j) + " " + (p.reverse ? "1 " : "0 ") + p.q + " " + p.r +
             ((p.q == p.r && !p.reverse) ? " 1" : " 0");
    return copy_out(out, buf, cap);
  } catch (std::string &s) {
    g_err = s;
    return -1;
  }
}

// the arguments behind `sedef seeds`, separated by newlines -> "k w u nbins extend_ratio max_extend merge_dist|seeds dir|pos..."
int sdfh_seeds_args(const char *args, char *buf, size_t cap) {
  try {
    std::vector<std::string> a = split(args, '\n');
    std::vector<char *> argv;
    for (auto &s : a) argv.push_back(&s[0]);
    const SeedsParams p = parse_seeds_args((int)argv.size(), argv.data());
    char head[256];
    snprintf(head, sizeof head, "%d %d %d %d %.17g %d %d", p.search.kmer_size, p.search.window_size, p.search.min_uppercase, p.nbins,
             p.bucket.extend_ratio, p.bucket.max_extend, p.bucket.merge_dist);
    std::string out = std::string(head) + "|" + p.seeds_dir;
    for (auto &s : p.search.pos) out += "|" + s;
    return copy_out(out, buf, cap);
  } catch (std::string &s) {
    g_err = s;
    return -1;
  }
}

// Hit::from_bed of a line as `align bucket` reads a seed: out = {query_start, query_end, ref_start, ref_end, query is_rc, ref is_rc};
// buf: "query name|reference name"
int sdfh_hit_from_bed(const char *line, int *out, char *buf, size_t cap) {
  try {
    const Hit h = Hit::from_bed(line);
    out[0] = h.query_start, out[1] = h.query_end, out[2] = h.ref_start, out[3] = h.ref_end, out[4] = h.query->is_rc, out[5] = h.ref->is_rc;
    return copy_out(h.query->name + "|" + h.ref->name, buf, cap);
  } catch (std::string &s) {
    g_err = s;
    return -1;
  }
}

}  // extern "C"
