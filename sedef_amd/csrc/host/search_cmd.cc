// `sedef search` and `sedef translate` (restates the CLI contract of reference src/search_main.cc:93-241): the pair loop over
// resident chromosomes and their search indexes (include/sedef_hip.h: sdf_search_index_build, sdf_search_pair_indexed; with
// SDF_SEARCH_LANES=N the pairs as one sdf_search_pairs_indexed call, N in flight), the BED
// text of a search hit, the translation groups, and the caller's table of the search entry points --
// relaxed_jaccard_estimate(query_size), src/util.cc:52-113 -- stated without Boost.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <set>

#include "../../../include/sedef_hip.h"
#include "search_run.h"
#include "sedef_host.h"

namespace sdfh {

// ---- the limit table ------------------------------------------------------------------------------------------------
double search_tau(double edit_error, int kmer_size, double max_error, double max_edit_error) {
  const double ratio = (max_error - max_edit_error) / max_edit_error;
  const double gap_error = std::min(1.0, ratio * edit_error);
  const double a = (1 - gap_error) / (1 + gap_error);
  const double b = 1 / (2 * std::exp(kmer_size * edit_error) - 1);
  return a * b;
}

// The edit error d in [0, 1] at which the expected Jaccard value is j: a Newton iteration from 0.10 that keeps a bracket.  The
// bracket closes on the side a step leaves; a step that has not halved within two iterations is replaced by half the way to
// the bracket's end, and so is one that would leave the bracket; the iteration ends when the step is below one part in 2^52
// of the value, or the function is exactly 0.
double solve_inverse_jaccard(double j, int kmer_size, double max_error, double max_edit_error) {
  if (j == 0) return 1;
  if (j == 1) return 0;
  const double ratio = (max_error - max_edit_error) / max_edit_error, k = kmer_size;
  double lo = 0.0, hi = 1.0, x = 0.10;
  const double eps = std::ldexp(1.0, 1 - 53);
  double delta = HUGE_VAL, delta1 = HUGE_VAL, delta2 = HUGE_VAL;
  for (int it = 0; it < 400; it++) {
    delta2 = delta1, delta1 = delta;
    const double E = std::exp(x * k);
    const double f = ((1 - x * ratio) / (1 + x * ratio)) * (1.0 / (2 * E - 1)) - j;
    const double g = 2 * (-k * E + ratio - 2 * ratio * E + E * k * std::pow(x * ratio, 2)) / std::pow((2 * E - 1) * (1 + x * ratio), 2);
    if (f == 0) break;
    if (g == 0) delta = f > 0 ? (x - hi) / 2 : (x - lo) / 2;  // (flat: towards the end the sign of f names; f decreases in x)
    else delta = f / g;
    if (std::fabs(delta * 2) > std::fabs(delta2)) {
      const double shift = delta > 0 ? (x - lo) / 2 : (x - hi) / 2;
      delta = (x != 0 && std::fabs(shift) > std::fabs(x)) ? std::copysign(std::fabs(x) * 1.1, delta) : shift;
      delta1 = delta2 = 3 * delta;
    }
    const double guess = x;
    x -= delta;
    if (x <= lo) {
      delta = 0.5 * (guess - lo), x = guess - delta;
      if (x == lo || x == hi) break;
    } else if (x >= hi) {
      delta = 0.5 * (guess - hi), x = guess - delta;
      if (x == lo || x == hi) break;
    }
    if (delta > 0) hi = guess;
    else lo = guess;
    if (!(std::fabs(x * eps) < std::fabs(delta))) break;
  }
  return x;
}

// the smallest x with P(X <= x) >= 1 - q for X ~ Binomial(s, p), by summing the mass function: the upper quantile at
// complement probability q, rounded outwards (up)
int binomial_upper_quantile(int s, double p, double q) {
  if (!(p > 0)) return 0;
  if (p >= 1) return s;
  const double target = 1 - q, odds = p / (1 - p);
  // mass(0) = (1 - p)^s may underflow for a large s * p: start in logarithms and sum from there
  double log_mass = s * std::log1p(-p), cum = 0;
  for (int x = 0; x <= s; x++) {
    cum += std::exp(log_mass);
    if (cum >= target) return x;
    log_mass += std::log((double)(s - x) / (x + 1) * odds);
  }
  return s;
}

namespace {
// the exit test of the reference's loop at `result`
bool estimate_exits(int s, int result, int kmer_size, double max_error, double max_edit_error) {
  const double Q2 = (1.0 - 0.75) / 2;
  const double d = solve_inverse_jaccard((double)result / s, kmer_size, max_error, max_edit_error);
  const double x = binomial_upper_quantile(s, search_tau(d, kmer_size, max_error, max_edit_error), Q2);
  const double low_d = solve_inverse_jaccard(x / s, kmer_size, max_error, max_edit_error);
  return 100 * (1 - low_d) < max_edit_error;
}
int estimate_top(int s, int kmer_size, double max_error, double max_edit_error) {
  return (int)std::ceil(s * search_tau(max_edit_error, kmer_size, max_error, max_edit_error));
}
}  // namespace

// the loop as the reference writes it: from ceil(s * tau(MAX_EDIT_ERROR)) down, one past the first result that passes
int relaxed_jaccard_estimate_walk(int s, int kmer_size, double max_error, double max_edit_error) {
  if (s < 1) return 0;
  int result = estimate_top(s, kmer_size, max_error, max_edit_error);
  for (; result >= 0; result--)
    if (estimate_exits(s, result, kmer_size, max_error, max_edit_error)) {
      result++;
      break;
    }
  return std::max(result, 0);
}

// The same value without the walk.  The exit test is monotone in `result` -- a larger result is a larger success probability and
// a larger quantile --: it holds up to some result and fails above it, so the first result the walk passes is the largest
// that passes, found by bisection (DESIGN.md states what this rests on; tests compare both forms).
int relaxed_jaccard_estimate(int s, int kmer_size, double max_error, double max_edit_error) {
  if (s < 1) return 0;
  const int top = estimate_top(s, kmer_size, max_error, max_edit_error);
  if (top < 0) return 0;
  if (!estimate_exits(s, 0, kmer_size, max_error, max_edit_error)) return 0;
  int lo = 0, hi = top + 1;  // passes at lo, fails at hi (or hi is beyond the walk's start)
  if (top >= 1 && !estimate_exits(s, 1, kmer_size, max_error, max_edit_error)) hi = 1;  // (the common case, in two tests)
  while (hi - lo > 1) {
    const int mid = lo + (hi - lo) / 2;
    if (estimate_exits(s, mid, kmer_size, max_error, max_edit_error)) lo = mid;
    else hi = mid;
  }
  // the guard: the walk starts at `top` and would stop there if it passed -- then the test was not monotone, and the walk decides
  if (lo + 1 < top && estimate_exits(s, top, kmer_size, max_error, max_edit_error))
    return relaxed_jaccard_estimate_walk(s, kmer_size, max_error, max_edit_error);
  return lo + 1;
}

const std::vector<int32_t> &LimitTable::upto(size_t n) {
  if (table_.empty()) table_.push_back(0);  // (limit[0] is never read)
  while (table_.size() < n) table_.push_back(relaxed_jaccard_estimate((int)table_.size(), kmer_size_, max_error_, max_edit_error_));
  return table_;
}

// one integer per line, line s (counted from 1) = limit[s]; empty lines at the end are allowed
std::vector<int32_t> read_limit_table(const std::string &path) {
  std::ifstream fin(path.c_str());
  if (!fin.is_open()) throw "Limit table " + path + " does not exist";
  std::vector<int32_t> t{0};
  bool ended = false;
  long long linenum = 0;
  for (std::string line; std::getline(fin, line);) {
    ++linenum;
    if (!line.empty() && line.back() == '\r') line.pop_back();
    if (line.empty()) {
      ended = true;
      continue;
    }
    char *end = nullptr;
    const long long v = strtoll(line.c_str(), &end, 10);
    if (ended || end == line.c_str() || *end)
      throw "Limit table " + path + ": line " + std::to_string(linenum) + " is not one integer";
    if (v < 1 || v > 0x7fffffff) throw "Limit table " + path + ": line " + std::to_string(linenum) + " is below 1 or beyond 2^31 - 1";
    t.push_back((int32_t)v);
  }
  if (t.size() < 2) throw "Limit table " + path + " is empty";
  return t;
}

// ---- translation groups (src/search_main.cc:93-120) ---------------------------------------------------------------------
std::vector<std::vector<std::string>> translation_groups(std::vector<std::pair<size_t, std::string>> records, int max_size) {
  std::sort(records.begin(), records.end(), std::greater<std::pair<size_t, std::string>>());
  std::vector<std::vector<std::string>> groups;
  int filled = 0;  // (an int in the reference as well)
  for (auto &c : records) {
    if (groups.empty() || filled + c.first > (size_t)max_size) {
      groups.push_back({c.second});
      filled = (int)c.first;
    } else {
      groups.back().push_back(c.second);
      filled += (int)c.first;
    }
  }
  return groups;
}

namespace {
struct FaiRecord {
  std::string key, name;
  long long length;   // the column as a 64-bit number: what `search` checks against 2^31 - 1
  size_t group_size;  // (size_t)atoi of the column: what the groups have always been formed from (`align bucket` reads them too)
};
// the records of genome.fa.fai, one per first word of a name (the first entry wins), in the order of those words
std::vector<FaiRecord> read_fai(const std::string &ref_path) {
  std::ifstream fai((ref_path + ".fai").c_str());
  if (!fai.is_open()) throw "Index file " + ref_path + ".fai does not exist";
  std::map<std::string, FaiRecord> by_key;
  for (std::string line; std::getline(fai, line);) {
    const auto f = split(line, '\t');
    if (f.size() != 5) throw "Index file " + ref_path + ".fai is malformed";
    const std::string key = split(f[0], ' ').at(0);
    by_key.insert({key, FaiRecord{key, f[0], strtoll(f[1].c_str(), nullptr, 10), (size_t)atoi(f[1].c_str())}});
  }
  std::vector<FaiRecord> out;
  for (auto &e : by_key) out.push_back(e.second);
  return out;
}
}  // namespace

std::vector<std::vector<std::string>> generate_translation(const std::string &ref_path, int max_size) {
  std::vector<std::pair<size_t, std::string>> records;
  for (auto &r : read_fai(ref_path)) records.push_back({r.group_size, r.name});
  return translation_groups(records, max_size);
}
std::vector<std::vector<std::string>> generate_translation(const std::string &ref_path) {
  return generate_translation(ref_path, 100 * 1000 * 1000);
}

int translate_command(const std::string &ref_path, FILE *out, FILE *log) {
  fprintf(log, "Translating %s...\n", ref_path.c_str());
  const auto groups = generate_translation(ref_path, stage_settings().translate_limit);
  for (size_t i = 0; i < groups.size(); i++) {
    std::string names;
    for (auto &n : groups[i]) names += (names.empty() ? "" : ", ") + n;
    fprintf(log, " [Translate] %zu -> %s\n", i, names.c_str());
  }
  fprintf(out, "%zu\n", groups.size());
  return 0;
}

// ---- the BED text of a search hit: Hit::to_bed() with its defaults on a hit without a name or an alignment and the
// comment "OK" (src/hit.cc:134-196, src/search.cc:256-258) ----
std::string search_hit_bed(const std::string &qname, const std::string &rname, int qs, int qe, int ref_start, int ref_end, bool ref_rc,
                           size_t ref_len) {
  // (size_t arithmetic brought to an int, as there; the + 1 is the reference's)
  const int rs = ref_rc ? (int)(ref_len - ref_end + 1) : ref_start;
  const int re = ref_rc ? (int)(ref_len - ref_start + 1) : ref_end;
  std::string out = qname + "\t" + std::to_string(qs) + "\t" + std::to_string(qe) + "\t" + rname + "\t" + std::to_string(rs) + "\t" +
                    std::to_string(re) + "\t\t\t+\t" + (ref_rc ? "-" : "+") + "\t" + std::to_string(std::max(qe - qs, ref_end - ref_start)) +
                    "\t0\t\t;OK";
  return out;
}

// ---- the arguments ----------------------------------------------------------------------------------------------------
// The reference's parser takes a value for the options it has registered and reads every other option as a flag; a token
// that is a number is never an option.  -l / --min-read-size is registered there and never read: its value is dropped here too.
SearchParams parse_search_options(int argc, char **argv) {
  static const char *const with_value[] = {"k", "kmer", "w", "window", "u", "uppercase", "e", "error", "E", "edit-error",
                                           "g", "gap-freq", "l", "min-read-size", "limit-table"};
  SearchParams p;
  auto is_number = [](const std::string &s) {
    char *e = nullptr;
    strtod(s.c_str(), &e);
    return !s.empty() && e && *e == 0;
  };
  auto number = [](const std::string &name, const std::string &v, bool integer) {
    char *e = nullptr;
    const double d = strtod(v.c_str(), &e);
    if (v.empty() || !e || *e || (integer && d != std::floor(d))) throw "Option " + name + ": " + v + " is not a number";
    return d;
  };
  for (int i = 0; i < argc; i++) {
    const std::string a = argv[i];
    if (!(a.size() > 1 && a[0] == '-' && !is_number(a))) {
      p.pos.push_back(a);
      continue;
    }
    std::string name = a.substr(a.find_first_not_of('-')), value;
    bool has_value = false;
    const size_t eq = name.find('=');
    if (eq != std::string::npos) value = name.substr(eq + 1), name = name.substr(0, eq), has_value = true;
    bool takes = false;
    for (const char *n : with_value) takes |= name == n;
    if (takes && !has_value) {
      if (i + 1 >= argc) throw "Option " + a + " needs a value";
      value = argv[++i];
    }
    if (name == "k" || name == "kmer") p.kmer_size = (int)number(a, value, true);
    else if (name == "w" || name == "window") p.window_size = (int)number(a, value, true);
    else if (name == "u" || name == "uppercase") p.min_uppercase = (int)number(a, value, true);
    else if (name == "e" || name == "error") p.max_error = number(a, value, false);
    else if (name == "E" || name == "edit-error") p.max_edit_error = number(a, value, false);
    else if (name == "g" || name == "gap-freq") p.gap_frequency = number(a, value, false);
    else if (name == "limit-table") p.limit_table = value;
    else if (name == "l" || name == "min-read-size") (void)value;
    else if (name == "t" || name == "transform") p.transform = true;
    else if (name == "r" || name == "reverse") p.reverse = true;
    else throw "Unknown option " + a;
  }
  p.min_read_size = (int)(1000 * (1 - p.max_error));  // KB * (1 - MAX_ERROR), in double as written
  return p;
}
SearchParams parse_search_args(int argc, char **argv) {
  SearchParams p = parse_search_options(argc, argv);
  if (p.pos.size() < 3) throw std::string("Not enough arguments to search");
  return p;
}


// ---- a run on one device context (search_run.h) -----------------------------------------------------------------------------
namespace {
std::map<std::string, long long> fai_lengths(const std::string &ref_path) {
  std::map<std::string, long long> out;
  for (auto &r : read_fai(ref_path)) out[r.key] = r.length;
  return out;
}
}  // namespace

SearchRun::SearchRun(const SearchParams &p, const std::string &ref_path, int device)
    : p_(p), fai_len_(fai_lengths(ref_path)), fr_(ref_path), computed_(p.kmer_size, p.max_error, p.max_edit_error) {
  memset(&P_, 0, sizeof P_);
  ctx_ = sdf_create(device, 0);
  if (!ctx_) throw std::string("no usable HIP device: ") + sdf_last_error(nullptr);
}
SearchRun::~SearchRun() { sdf_destroy(ctx_); }

void SearchRun::check(int rc, const char *what) const {
  if (rc != SDF_OK) throw std::string(what) + ": " + sdf_last_error(ctx_);
}

void SearchRun::upload(const std::string &name) {
  if (chroms_.count(name)) return;
  const auto it = fai_len_.find(name);
  if (it == fai_len_.end()) throw "Chromosome " + name + " does not exist";
  if (it->second > 0x7fffffffLL) throw "Chromosome " + name + " is longer than 2^31 - 1 bases: not supported";
  const FastaReference::Record rec = fr_.record(name);
  int64_t off = 0;
  check(sdf_pool_append_fasta(ctx_, rec.bytes, rec.nbytes, rec.entry->length, rec.entry->line_blen, rec.entry->line_len, chroms_.empty(), &off),
        "sdf_pool_append_fasta");
  chroms_[name] = Chrom{off, (int32_t)rec.entry->length};
}
void SearchRun::uploaded() { check(sdf_pool_sync(ctx_), "sdf_pool_sync"); }

void SearchRun::index(const std::string &name, bool rc) {
  if (indices_.count({name, rc})) return;
  const sdf_minim_range range{chroms_.at(name).off, chroms_.at(name).len, rc ? SDF_MINIM_RC : 0};
  sdf_search_index *h = nullptr;
  check(sdf_search_index_build(ctx_, &range, p_.kmer_size, p_.window_size, p_.separate_lowercase, &h), "sdf_search_index_build");
  indices_[{name, rc}] = h;
}

void SearchRun::prepare(const std::vector<std::string> &queries) {
  size_t most = 0;  // the most minimizers a query has: no window holds more
  for (auto &q : queries) {
    sdf_search_index_desc d;
    check(sdf_search_index_info(ctx_, indices_.at({q, false}), &d), "sdf_search_index_info");
    most = std::max(most, (size_t)d.n_minimizers);
  }
  if (!p_.limit_table.empty()) given_ = read_limit_table(p_.limit_table);
  const std::vector<int32_t> &limit = given_.empty() ? computed_.upto(most + 1) : given_;
  if (!given_.empty() && given_.size() < most + 1)
    throw "Limit table " + p_.limit_table + " has " + std::to_string(given_.size() - 1) + " lines; this run needs " + std::to_string(most);
  for (size_t s = 1; s < limit.size(); s++)
    if (limit[s] < 1) throw "The limit table has " + std::to_string(limit[s]) + " at " + std::to_string(s) + ": the search needs 1 or more";
  limit_ = &limit;
  memset(&P_, 0, sizeof P_);
  P_.k = p_.kmer_size, P_.w = p_.window_size, P_.separate_lowercase = p_.separate_lowercase, P_.uppercase_seeds = p_.uppercase_seeds;
  P_.min_read_size = p_.min_read_size;
  P_.filter.min_uppercase = p_.min_uppercase, P_.filter.max_error = p_.max_error, P_.filter.max_edit_error = p_.max_edit_error;
  P_.filter.gap_frequency = p_.gap_frequency;
  P_.extend.max_error = p_.max_error, P_.extend.max_edit_error = p_.max_edit_error, P_.extend.max_sd_size = p_.max_sd_size;
  P_.limit = limit.data(), P_.n_limit = limit.size();
}

void SearchRun::run(const std::vector<SearchPair> &pairs, int n_lanes, std::vector<sdf_search_pair_hit> &hits, std::vector<uint64_t> &first) {
  const size_t n_wide = (size_t)stage_settings().search_wide;
  first.assign(pairs.size() + 1, 0);
  if (n_lanes > 1) {
    // SDF_SEARCH_LANES=N: every pair as one job of one call, N of them in flight; the hits in the pairs' order
    sdf_search_lanes *lanes = nullptr;
    check(sdf_search_lanes_open(ctx_, n_lanes, &lanes), "sdf_search_lanes_open");
    std::vector<sdf_search_pair_job> jobs;
    for (auto &pr : pairs)
      jobs.push_back(sdf_search_pair_job{indices_.at({pr.q, false}), indices_.at({pr.r, pr.reverse}), (pr.q == pr.r) && !pr.reverse, 0});
    std::vector<sdf_search_pair_stats> stats(jobs.size());
    // (an overflow costs a second run of EVERY pair, where the loop repeats one: room for 4,096 hits a pair from the start)
    hits.resize(std::max<size_t>(1024, 4096 * jobs.size()));
    size_t used = 0;
    int rc = sdf_search_pairs_indexed(ctx_, lanes, jobs.data(), jobs.size(), &P_, n_wide, hits.data(), hits.size(), &used, first.data(), stats.data());
    if (rc == SDF_ERR_CIGAR_OVERFLOW) {
      hits.resize(used + used / 2);
      rc = sdf_search_pairs_indexed(ctx_, lanes, jobs.data(), jobs.size(), &P_, n_wide, hits.data(), hits.size(), &used, first.data(), stats.data());
    }
    check(rc, "sdf_search_pairs_indexed");
    check(sdf_search_lanes_close(ctx_, lanes), "sdf_search_lanes_close");
    hits.resize(used);
    for (auto &st : stats) attempted_ += st.attempted, jaccard_failed_ += st.jaccard_failed, interval_failed_ += st.interval_failed;
  } else {
    hits.clear();
    std::vector<sdf_search_pair_hit> one(1024);
    for (size_t j = 0; j < pairs.size(); j++) {
      const SearchPair &pr = pairs[j];
      P_.same_genome = (pr.q == pr.r) && !pr.reverse;
      P_.extend.same_genome = P_.same_genome;
      const sdf_search_index *qh = indices_.at({pr.q, false}), *rh = indices_.at({pr.r, pr.reverse});
      size_t used = 0;
      sdf_search_pair_stats st;
      // (SDF_SEARCH_WIDE_DEVICE=N: the seeding's WIDE / FOUND_WIDE windows on the device; 0 is sdf_search_pair_indexed itself)
      int rc = sdf_search_pair_indexed_wide(ctx_, qh, rh, &P_, one.data(), one.size(), &used, &st, n_wide);
      if (rc == SDF_ERR_CIGAR_OVERFLOW) {
        one.resize(used + used / 2);
        rc = sdf_search_pair_indexed_wide(ctx_, qh, rh, &P_, one.data(), one.size(), &used, &st, n_wide);
      }
      check(rc, "sdf_search_pair_indexed");
      hits.insert(hits.end(), one.begin(), one.begin() + (long)used);
      first[j + 1] = hits.size();
      attempted_ += st.attempted, jaccard_failed_ += st.jaccard_failed, interval_failed_ += st.interval_failed;
    }
  }
  total_ += (long long)hits.size(), pairs_ += (long long)pairs.size();
}

std::string SearchRun::bed(const SearchPair &pair, const sdf_search_pair_hit &h) const {
  return search_hit_bed(pair.q, pair.r, h.query_start, h.query_end, h.ref_start, h.ref_end, pair.reverse, (size_t)chroms_.at(pair.r).len);
}

void SearchRun::log_totals(FILE *log, int n_lanes, double seconds) const {
  fprintf(log, "Total:           = %10lld\n", total_);
  fprintf(log, "Fails: attempts  = %10lld\n       Jaccard   = %10lld\n       interval  = %10lld\n", attempted_, jaccard_failed_, interval_failed_);
  const std::string in_lanes = n_lanes > 1 ? ", " + std::to_string(n_lanes) + " lanes" : "";  // (lanes build no index: the counts stay)
  fprintf(log, "Indexes built: %lld for %lld pairs%s (%zu chromosomes resident, limit table of %zu entries) in %.1fs\n",
          sdf_search_index_builds(ctx_), pairs_, in_lanes.c_str(), chroms_.size(), limit_ ? limit_->size() - 1 : (size_t)0, seconds);
}

void log_search_parameters(const SearchParams &p, FILE *log) {
  fprintf(log,
          "        Parameters: READ_SIZE      = %d\n"
          "                    MAX_ERROR      = %.2f (%.2f EDIT + %.2f GAP; GAPFREQ=%.3f)\n",
          p.min_read_size, p.max_error, p.max_edit_error, p.max_error - p.max_edit_error, p.gap_frequency);
}

// ---- the command ------------------------------------------------------------------------------------------------------
int search_command(const SearchParams &p, FILE *out, FILE *log) {
  using Clock = std::chrono::steady_clock;
  log_search_parameters(p, log);
  fprintf(log, "Reverse complement: %s\nk-mer size:         %d\nWindow size:        %d\n\n", p.reverse ? "true" : "false", p.kmer_size,
          p.window_size);
  auto T = Clock::now();
  const std::string &ref_path = p.pos[0];
  std::vector<std::string> qr, rr;
  if (!p.transform) {
    qr.push_back(p.pos[1]);
    rr.push_back(p.pos[2]);
  } else {
    const auto groups = generate_translation(ref_path, stage_settings().translate_limit);
    for (int side = 0; side < 2; side++) {
      char *e = nullptr;
      const long g = strtol(p.pos[1 + side].c_str(), &e, 10);
      if (e == p.pos[1 + side].c_str() || *e || g < 0 || (size_t)g >= groups.size())
        throw "Translation group " + p.pos[1 + side] + " does not exist (" + std::to_string(groups.size()) + " groups)";
      for (auto &name : groups[(size_t)g]) (side ? rr : qr).push_back(split(name, ' ').at(0));
    }
  }
  // every chromosome the run names goes to the device once
  SearchRun R(p, ref_path, stage_settings().device);
  for (auto &r : rr) R.upload(r);
  for (auto &q : qr) R.upload(q);
  R.uploaded();
  // one index per (name, strand): the references on the strand of -r, then the queries that are not there yet, forward
  for (auto &r : rr) R.index(r, p.reverse);
  for (auto &q : qr) R.index(q, false);
  fprintf(log, "Building index took %.1fs\n", std::chrono::duration<double>(Clock::now() - T).count());
  T = Clock::now();
  R.prepare(qr);
  std::vector<SearchPair> pairs;
  for (auto &r : rr)
    for (auto &q : qr) pairs.push_back(SearchPair{q, r, p.reverse});
  const int n_lanes = stage_settings().search_lanes;
  std::vector<sdf_search_pair_hit> hits;
  std::vector<uint64_t> first;
  R.run(pairs, n_lanes, hits, first);
  std::string text;
  for (size_t j = 0; j < pairs.size(); j++) {
    text.clear();
    for (size_t i = (size_t)first[j]; i < (size_t)first[j + 1]; i++) text += R.bed(pairs[j], hits[i]) + "\n";
    fwrite(text.data(), 1, text.size(), out);
  }
  fflush(out);
  R.log_totals(log, n_lanes, std::chrono::duration<double>(Clock::now() - T).count());
  return 0;
}

}  // namespace sdfh
