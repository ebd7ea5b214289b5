// `sedef seeds`: the seeding phase of sedef.sh (:133-140, two `sedef search [-r] -t i j` processes per unordered pair of
// translation groups) and its `sedef align bucket` (:169) in ONE process and one device context.  Every chromosome is uploaded
// once and indexed once per strand (search_run.h: SearchRun, which `sedef search` runs on too); the pairs of all jobs go through
// one SearchRun::run; their hits never become text on the way to the buckets: sdf_seeds_bucket_merge (include/sedef_hip.h) turns
// them into seed records and merges them on the device, and the bucket files are written from its records as `align bucket`
// writes them with SDF_BUCKET_DEVICE=1 (bucket.cc).  --seeds-dir also leaves the files the search processes would have left.
// Where the records path cannot take the run, the same hits are bucketed from their BED text on the host path, said in one line.
#include <sys/stat.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <sstream>

#include "search_run.h"

namespace sdfh {

std::vector<SeedsPair> seeds_pairs(const std::vector<std::vector<std::string>> &groups) {
  std::vector<SeedsPair> out;
  const int G = (int)groups.size();
  for (int j = 0; j < G; j++)        // reference
    for (int i = j; i < G; i++)      // query
      for (int m = 0; m < 2; m++)    // n, y
        for (auto &r : groups[(size_t)j])
          for (auto &q : groups[(size_t)i]) out.push_back(SeedsPair{i, j, m == 1, split(q, ' ').at(0), split(r, ' ').at(0)});
  return out;
}

// The options of `align bucket` and --seeds-dir are taken out; what remains is `sedef search`'s (parse_search_options).
SeedsParams parse_seeds_args(int argc, char **argv) {
  static const char *const own[] = {"n", "bins", "extend-ratio", "max-extend", "merge-dist", "seeds-dir"};
  SeedsParams sp;
  std::vector<char *> rest;
  bool have_bins = false;
  for (int i = 0; i < argc; i++) {
    const std::string a = argv[i];
    std::string name = a.size() > 1 && a[0] == '-' ? a.substr(a.find_first_not_of('-')) : "", value;
    const size_t eq = name.find('=');
    const bool has_value = eq != std::string::npos;
    if (has_value) value = name.substr(eq + 1), name = name.substr(0, eq);
    bool mine = false;
    for (const char *n : own) mine |= name == n;
    if (!mine) {
      rest.push_back(argv[i]);
      continue;
    }
    if (!has_value) {
      if (i + 1 >= argc) throw "Option " + a + " needs a value";
      value = argv[++i];
    }
    if (name == "n" || name == "bins") sp.nbins = atoi(value.c_str()), have_bins = true;
    else if (name == "extend-ratio") sp.bucket.extend_ratio = atof(value.c_str());
    else if (name == "max-extend") sp.bucket.max_extend = atoi(value.c_str());
    else if (name == "merge-dist") sp.bucket.merge_dist = atoi(value.c_str());
    else sp.seeds_dir = value;
  }
  sp.search = parse_search_options((int)rest.size(), rest.data());
  if (sp.search.reverse || sp.search.transform)
    throw std::string("sedef seeds runs both strands and all groups: -r and -t are not taken");
  if (!have_bins) throw std::string("Must provide number of bins (--bins)");
  if (sp.search.pos.size() < 2) throw std::string("Not enough arguments to seeds");
  return sp;
}

int seeds_command(const SeedsParams &sp, FILE *log) {
  using Clock = std::chrono::steady_clock;
  const SearchParams &p = sp.search;
  log_search_parameters(p, log);
  fprintf(log, "Reverse complement: both\nk-mer size:         %d\nWindow size:        %d\n\n", p.kmer_size, p.window_size);
  auto T = Clock::now();
  const std::string &ref_path = p.pos[0], &output_dir = p.pos[1];
  const auto groups = generate_translation(ref_path, stage_settings().translate_limit);
  const std::vector<SeedsPair> all = seeds_pairs(groups);
  std::vector<std::string> names;  // every chromosome of the run ...
  for (auto &g : groups)
    for (auto &name : g) names.push_back(split(name, ' ').at(0));
  SearchRun R(p, ref_path, stage_settings().device);
  for (auto &name : names) R.upload(name);
  R.uploaded();
  for (auto &name : names) R.index(name, false), R.index(name, true);
  fprintf(log, "Building index took %.1fs\n", std::chrono::duration<double>(Clock::now() - T).count());
  T = Clock::now();
  R.prepare(names);
  std::vector<SearchPair> pairs;
  for (auto &pr : all) pairs.push_back(SearchPair{pr.q, pr.r, pr.reverse});
  const int n_lanes = stage_settings().search_lanes;
  std::vector<sdf_search_pair_hit> hits;
  std::vector<uint64_t> first;
  R.run(pairs, n_lanes, hits, first);
  R.log_totals(log, n_lanes, std::chrono::duration<double>(Clock::now() - T).count());

  // the files of sedef.sh: <i>_<j>_<n|y>.bed holds the lines of its pairs in their order (a job without hits: an empty file)
  const auto job_files = [&] {
    std::vector<std::pair<std::string, std::string>> files;
    for (size_t k = 0; k < all.size(); k++) {
      const std::string name = std::to_string(all[k].i) + "_" + std::to_string(all[k].j) + "_" + (all[k].reverse ? "y" : "n") + ".bed";
      if (files.empty() || files.back().first != name) files.emplace_back(name, "");
      for (size_t t = (size_t)first[k]; t < (size_t)first[k + 1]; t++) files.back().second += R.bed(pairs[k], hits[t]) + "\n";
    }
    return files;
  };
  if (!sp.seeds_dir.empty()) {
    mkdir(sp.seeds_dir.c_str(), 0777);  // (one that exists stays)
    for (auto &f : job_files()) {
      FILE *out = fopen((sp.seeds_dir + "/" + f.first).c_str(), "w");
      if (!out) throw "Cannot open file " + sp.seeds_dir + "/" + f.first + " for writing";
      fwrite(f.second.data(), 1, f.second.size(), out);
      fclose(out);
    }
  }
  mkdir(output_dir.c_str(), 0777);

  // ... numbered in the order of the names, a table entry per pair, and the chain on the device
  std::sort(names.begin(), names.end());
  std::string why;
  BucketTables tab;
  if (!bucket_tables(names, ref_path, &tab)) why = "more than 4096 chromosome groups or 2^19 chromosomes";
  if (why.empty()) {
    std::map<std::string, int32_t> id_of;
    for (size_t c = 0; c < names.size(); c++) id_of[names[c]] = (int32_t)c;
    std::vector<sdf_seed_job> jobs;
    for (auto &pr : pairs) jobs.push_back(sdf_seed_job{id_of.at(pr.q), id_of.at(pr.r), (int64_t)R.length(pr.r), pr.reverse ? SDF_SEED_RC : 0u, 0u});
    const sdf_bucket_params P{sp.bucket.extend_ratio, sp.bucket.max_extend, sp.bucket.merge_dist, sp.nbins};
    std::vector<sdf_bucket_hit> out(hits.size());
    size_t n_out = 0, n_dropped = 0;
    const int rc = sdf_seeds_bucket_merge(R.ctx(), hits.data(), hits.size(), first.data(), jobs.data(), jobs.size(), tab.chr_group.data(),
                                          tab.chr_group.size(), tab.pair_order.data(), tab.n_groups, &P, out.data(), out.size(), &n_out, &n_dropped);
    if (rc == SDF_ERR_INVALID || rc == SDF_ERR_UNSUPPORTED) why = sdf_last_error(R.ctx());
    else R.check(rc, "sdf_seeds_bucket_merge");
    if (why.empty() && n_dropped)
      why = std::to_string(n_dropped) + " hits or table entries outside what sdf_bucket_merge_device takes (a coordinate below 0 or too large)";
    if (why.empty()) {
      fprintf(log, "\nRead total %d alignments\n", (int)hits.size());
      fprintf(log, "\nFinished with sorting\n");
      write_bucket_records(names, out.data(), n_out, sp.nbins, output_dir);
      return 0;
    }
  }
  fprintf(stderr, "[sedef_amd] sedef seeds: the records path ignored: %s, the host path buckets this run\n", why.c_str());
  auto files = job_files();
  std::sort(files.begin(), files.end());  // (the order `align bucket` reads a directory in: that of the names)
  bucket_alignments_streams(
      [&](const SeedStreamVisitor &visit) {
        for (auto &f : files) {
          std::istringstream lines(f.second);
          visit(sp.seeds_dir.empty() ? f.first : sp.seeds_dir + "/" + f.first, lines);
        }
      },
      sp.nbins, output_dir, true, ref_path, sp.bucket, log);
  return 0;
}

}  // namespace sdfh
