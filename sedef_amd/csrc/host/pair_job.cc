// fast_align + refine_chains as a resumable per-pair job (restates reference src/chain.cc:203-268, src/refine.cc:23-193).
#include <set>

#include "stage_internal.h"

namespace sdfh {

std::atomic<long long> g_us_chain(0), g_us_rest(0);
namespace {
struct ScopedUs {
  std::atomic<long long> &acc;
  Clock::time_point t0 = Clock::now();
  explicit ScopedUs(std::atomic<long long> &a) : acc(a) {}
  ~ScopedUs() { acc += std::chrono::duration_cast<std::chrono::microseconds>(Clock::now() - t0).count(); }
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

}  // namespace sdfh
