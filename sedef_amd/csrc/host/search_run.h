// What `sedef search` and `sedef seeds` share of a run on one device context (search_cmd.cc), and what `align bucket` and
// `sedef seeds` share of the records path (bucket.cc).  Internal to the host library: the declarations that name types of the
// C ABI (include/sedef_hip.h), which sedef_host.h does not include.
#pragma once
#include <map>
#include <string>
#include <vector>

#include "../../../include/sedef_hip.h"
#include "sedef_host.h"

namespace sdfh {

// One device context of a search run: every chromosome it is told of uploaded once, one index per (chromosome, strand), the
// limit table and the parameters of the pair calls, the pairs themselves -- SDF_SEARCH_LANES=N: as jobs of one
// sdf_search_pairs_indexed call, else one sdf_search_pair_indexed_wide call after the other -- and the totals of the log.
struct SearchPair {
  std::string q, r;
  bool reverse;  // the reference's index is on this strand, the query's is forward; same_genome = (q == r) && !reverse
};
class SearchRun {
 public:
  SearchRun(const SearchParams &p, const std::string &ref_path, int device);
  ~SearchRun();  // (destroys the context with the handles still live: include/sedef_hip.h)
  SearchRun(const SearchRun &) = delete;
  SearchRun &operator=(const SearchRun &) = delete;
  void upload(const std::string &name);  // a name twice is one upload
  void uploaded();                       // behind the last upload, before the first index
  void index(const std::string &name, bool rc);
  // the caller's table, sized up front: limit[s] for every s a window of a query of `queries` can have; and the parameters
  void prepare(const std::vector<std::string> &queries);
  // hits[first[j], first[j + 1]) are pair j's, in the order of `pairs`
  void run(const std::vector<SearchPair> &pairs, int n_lanes, std::vector<sdf_search_pair_hit> &hits, std::vector<uint64_t> &first);
  std::string bed(const SearchPair &pair, const sdf_search_pair_hit &h) const;  // search_hit_bed of a hit of `pair`
  int32_t length(const std::string &name) const { return chroms_.at(name).len; }
  sdf_ctx *ctx() const { return ctx_; }
  void check(int rc, const char *what) const;  // throws the context's error text
  void log_totals(FILE *log, int n_lanes, double seconds) const;  // "Total / Fails / Indexes built"

 private:
  struct Chrom {
    int64_t off;
    int32_t len;
  };
  SearchParams p_;
  sdf_ctx *ctx_ = nullptr;
  std::map<std::string, long long> fai_len_;
  FastaReference fr_;
  std::map<std::string, Chrom> chroms_;
  std::map<std::pair<std::string, bool>, sdf_search_index *> indices_;
  LimitTable computed_;
  std::vector<int32_t> given_;
  const std::vector<int32_t> *limit_ = nullptr;
  sdf_search_pair_params P_;
  long long total_ = 0, attempted_ = 0, jaccard_failed_ = 0, interval_failed_ = 0, pairs_ = 0;
};

void log_search_parameters(const SearchParams &p, FILE *log);  // the "Parameters:" block of the log

// ---- the records path of `align bucket` (bucket.cc) ----
// The two tables sdf_bucket_merge takes beside its records, for chromosomes numbered in the order of `names` (sorted: std::string
// compares bytes).  false: more groups or chromosomes than the call takes.
struct BucketTables {
  std::vector<int32_t> chr_group, pair_order;
  size_t n_groups = 1;
};
bool bucket_tables(const std::vector<std::string> &names, const std::string &reference, BucketTables *t);
// the bucket files from the records of a merge call: record j goes to file out[j].bucket, in this order
void write_bucket_records(const std::vector<std::string> &names, const sdf_bucket_hit *out, size_t n_out, int nbins, const std::string &output_dir);

}  // namespace sdfh
