// `sedef align bucket`: seed hits -> N bucket files for `align generate` (what bucket_alignments_extern of the reference
// produces, src/align_main.cc:38-198, with merge() of src/merge.cc:35-109 and the chromosome grouping of
// src/search_main.cc:93-120).
//
// The reference spills the extended seeds into one temporary file per pair of chromosome groups, re-reads each file to
// merge it, writes it back, and re-reads everything a third time to deal the hits into the buckets.  Here the seeds
// stream through memory once: they are grouped under the temporary file's NAME (its lexicographic order is the order the
// reference processes the groups in), every group is merged in place, and the hits are dealt straight into the bucket
// files.  A hit still passes through its BED text between the steps, exactly where the reference writes and re-reads it
// (the round trip drops fields: a seed's 14th column becomes the jaccard count, the CIGAR column is ignored).
#include <glob.h>
#include <sys/stat.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <functional>
#include <istream>
#include <map>
#include <tuple>

#include "search_run.h"

namespace sdfh {

namespace {
// a hit is kept with the pair ordered by (chromosome, start, end) of its two sides (src/merge.cc:38-46,
// src/align_main.cc:79-84); only the names, not the Sequence objects, change sides
void order_sides(Hit &h) {
  if (std::tie(h.query->name, h.query_start, h.query_end) > std::tie(h.ref->name, h.ref_start, h.ref_end)) {
    std::swap(h.query->name, h.ref->name);
    std::swap(h.query_start, h.ref_start);
    std::swap(h.query_end, h.ref_end);
  }
}

int complexity_class(const Hit &h) {  // src/align_main.cc:128-130, :172-174
  return (int)std::sqrt(double(h.query_end - h.query_start) * double(h.ref_end - h.ref_start)) / 1000;
}
int complexity_of(const Hit &h) {
  return (int)std::sqrt(double(h.query_end - h.query_start) * double(h.ref_end - h.ref_start));
}
}  // namespace

// Sweep over the hits in (strand, query chromosome, reference chromosome, query start, reference start) order.  The
// hits of the current run of nearby query intervals are kept as "windows" keyed by their reference end; a new hit
// swallows every window it comes within `merge_dist` of (in both sequences), repeatedly, as its own extent grows.
std::vector<Hit> merge_hits(std::vector<Hit> &hits, int merge_dist) {
  for (auto &h : hits) order_sides(h);
  // (std::sort, this comparator, this input order: equal keys end up where the reference's sort leaves them)
  std::sort(hits.begin(), hits.end(), [](const Hit &a, const Hit &b) {
    return std::tie(a.ref->is_rc, a.query->name, a.ref->name, a.query_start, a.ref_start) <
           std::tie(b.ref->is_rc, b.query->name, b.ref->name, b.query_start, b.ref_start);
  });
  std::vector<Hit> merged;
  std::multimap<int, Hit> windows;  // by reference end
  auto flush = [&] {
    for (auto &w : windows) merged.push_back(w.second);
    windows.clear();
  };
  auto apart = [&](const Hit &w, const Hit &h) {
    return w.query_end + merge_dist < h.query_start || w.ref_end < h.ref_start - merge_dist ||
           w.ref_start > h.ref_end + merge_dist;
  };
  Hit last;  // the previous hit, its query end raised to that of everything before it in the run (src/merge.cc:101-102)
  bool have_last = false;
  for (Hit &h : hits) {
    const bool self = h.query->name == h.ref->name && h.query_start == h.ref_start && h.query_end == h.ref_end &&
                      h.query->is_rc == h.ref->is_rc;
    if (self) continue;  // a region against itself
    const bool new_run = !have_last || last.query_end + merge_dist < h.query_start ||
                         last.query->name != h.query->name || last.ref->name != h.ref->name ||
                         last.ref->is_rc != h.ref->is_rc;
    if (new_run) {
      flush();
    } else {
      for (bool grew = true; grew;) {
        grew = false;
        for (auto w = windows.lower_bound(h.ref_start - merge_dist); w != windows.end();) {
          if (apart(w->second, h)) {
            ++w;
            continue;
          }
          h.query_start = std::min(h.query_start, w->second.query_start);
          h.query_end = std::max(h.query_end, w->second.query_end);
          h.ref_start = std::min(h.ref_start, w->second.ref_start);
          h.ref_end = std::max(h.ref_end, w->second.ref_end);
          w = windows.erase(w);
          grew = true;
        }
      }
    }
    windows.emplace(h.ref_end, h);
    if (!new_run) h.query_end = std::max(h.query_end, last.query_end);
    last = h;
    have_last = true;
  }
  flush();
  return merged;
}

// (generate_translation, the chromosome groups of `-t`: search_cmd.cc)

static std::vector<std::string> seed_files(const std::string &path) {  // src/align_main.cc:44-62
  struct stat st;
  if (stat(path.c_str(), &st) != 0) throw "Path " + path + " is neither file nor directory";
  std::vector<std::string> files;
  if (S_ISREG(st.st_mode)) {
    files.push_back(path);
  } else if (S_ISDIR(st.st_mode)) {
    glob_t g;
    glob((path + "/*.bed").c_str(), GLOB_TILDE, nullptr, &g);
    for (size_t i = 0; i < g.gl_pathc; i++) {
      struct stat s2;
      if (stat(g.gl_pathv[i], &s2) == 0 && S_ISREG(s2.st_mode)) files.push_back(g.gl_pathv[i]);
    }
    globfree(&g);
  } else {
    throw "Path " + path + " is neither file nor directory";
  }
  return files;
}

// The two tables sdf_bucket_merge takes beside its records (include/sedef_hip.h), for chromosomes numbered in the order of `names`
// (sorted: std::string compares bytes): the group of each by generate_translation(reference), and the order the reference reads its
// temporary files in -- that of their names.  false: more groups or chromosomes than the call takes.
bool bucket_tables(const std::vector<std::string> &names, const std::string &reference, BucketTables *t) {
  std::map<std::string, int> id_of;
  for (size_t i = 0; i < names.size(); i++) id_of[names[i]] = (int)i;
  const auto groups = generate_translation(reference);
  const size_t n_groups = std::max<size_t>(groups.size(), 1);
  if (n_groups > 4096 || names.size() > ((size_t)1 << 19)) return false;
  t->n_groups = n_groups;
  t->chr_group.assign(names.size(), 0);  // (a chromosome the index does not hold: group 0, as group_of[] answers)
  for (size_t g = 0; g < groups.size(); g++)
    for (auto &name : groups[g])
      if (id_of.count(name)) t->chr_group[(size_t)id_of[name]] = (int32_t)g;
  t->pair_order.assign(n_groups * n_groups, 0);
  std::vector<std::pair<std::string, int32_t>> tmp;
  for (size_t a = 0; a < n_groups; a++)
    for (size_t b = 0; b < n_groups; b++) tmp.emplace_back("tmp_" + std::to_string(a) + "_" + std::to_string(b) + ".tmp", (int32_t)(a * n_groups + b));
  std::sort(tmp.begin(), tmp.end());
  for (size_t k = 0; k < tmp.size(); k++) t->pair_order[(size_t)tmp[k].second] = (int32_t)k;
  return true;
}

static std::vector<FILE *> open_buckets(int nbins, const std::string &output_dir) {
  std::vector<FILE *> files;
  for (int b = 0; b < nbins; b++) {
    char name[64];
    snprintf(name, sizeof name, "/bucket_%04d", b);
    FILE *f = fopen((output_dir + name).c_str(), "w");
    if (!f) throw "Cannot open file " + output_dir + name + " for writing";
    files.push_back(f);
  }
  return files;
}

// The bucket files from the records of a merge call, out[0, n_out) in deal order: record j goes to file out[j].bucket.
void write_bucket_records(const std::vector<std::string> &names, const sdf_bucket_hit *out, size_t n_out, int nbins, const std::string &output_dir) {
  std::vector<FILE *> files = open_buckets(nbins, output_dir);
  std::vector<std::shared_ptr<Sequence>> fwd(names.size()), rev(names.size());  // a chromosome's name on either strand
  const auto side = [&](int32_t id, bool is_rc) {
    std::shared_ptr<Sequence> &s = (is_rc ? rev : fwd)[(size_t)id];
    if (!s) s = std::make_shared<Sequence>(names[(size_t)id], "", is_rc);
    return s;
  };
  for (size_t j = 0; j < n_out; j++) {
    const sdf_bucket_hit &r = out[j];
    Hit h;
    h.query = side(r.q_chr, false);
    h.ref = side(r.r_chr, (r.flags & SDF_SEED_RC) != 0);
    h.query_start = r.q_start, h.query_end = r.q_end, h.ref_start = r.r_start, h.ref_end = r.r_end;
    fputs(h.to_bed(false).c_str(), files[(size_t)r.bucket]);
    fputs("\n", files[(size_t)r.bucket]);
  }
  for (auto f : files) fclose(f);
}

// SDF_BUCKET_DEVICE=1: the seeds as records through ONE sdf_bucket_merge call (include/sedef_hip.h; form 2: through
// sdf_bucket_merge_host, no device) and the bucket files from its records.  The records hold coordinates, ids and the strand of
// the reference side and nothing else, which is all that survives of a seed as `sedef search` writes it (no name, forward
// query; the comment and the jaccard column are lost in the BED round trips of the host path): any other seed keeps the whole
// run on the host path -- false, with one line on stderr.
bool bucket_alignments_records(const std::string &bed_path, int nbins, const std::string &output_dir, const std::string &reference,
                               const BucketParams &bp, FILE *log, int form, int device) {
  const auto ignored = [](const std::string &why) {
    fprintf(stderr, "[sedef_amd] SDF_BUCKET_DEVICE=1 ignored: %s, the host path buckets this run\n", why.c_str());
    return false;
  };
  // the seeds, and the chromosomes numbered in the order of their names (std::string compares bytes)
  std::vector<Hit> seeds;
  std::vector<std::pair<std::string, int>> read;
  std::map<std::string, int> id_of;
  for (auto &file : seed_files(bed_path)) {
    std::ifstream fin(file.c_str());
    if (!fin.is_open()) throw "BED file " + bed_path + " does not exist";
    int count = 0;
    for (std::string line; std::getline(fin, line); count++) {
      seeds.push_back(Hit::from_bed(line));
      const Hit &h = seeds.back();
      if (!h.name.empty() || h.query->is_rc) return ignored("a seed with a name or a reverse query strand (" + file + ")");
      id_of[h.query->name] = 0, id_of[h.ref->name] = 0;
    }
    read.emplace_back(file, count);
  }
  std::vector<std::string> names;
  for (auto &kv : id_of) kv.second = (int)names.size(), names.push_back(kv.first);
  BucketTables tab;
  if (!bucket_tables(names, reference, &tab)) return ignored("more than 4096 chromosome groups or 2^19 chromosomes");
  const std::vector<int32_t> &chr_group = tab.chr_group, &pair_order = tab.pair_order;
  const size_t n_groups = tab.n_groups;
  std::vector<sdf_seed_hit> in(seeds.size());
  for (size_t i = 0; i < seeds.size(); i++) {
    const Hit &h = seeds[i];
    in[i] = sdf_seed_hit{id_of[h.query->name], h.query_start, h.query_end, id_of[h.ref->name], h.ref_start, h.ref_end, h.ref->is_rc ? SDF_SEED_RC : 0u, 0u};
  }
  seeds.clear();
  const sdf_bucket_params P{bp.extend_ratio, bp.max_extend, bp.merge_dist, nbins};
  std::vector<sdf_bucket_hit> out(in.size());
  size_t n_out = 0;
  if (form == 2) {
    if (sdf_bucket_merge_host(in.data(), in.size(), chr_group.data(), chr_group.size(), pair_order.data(), n_groups, &P, out.data(), out.size(), &n_out))
      return ignored("sdf_bucket_merge_host does not take these seeds or parameters");
  } else {
    sdf_ctx *ctx = sdf_create(device, 0);
    if (!ctx) throw std::string("no usable HIP device: ") + sdf_last_error(nullptr);
    const int rc = sdf_bucket_merge(ctx, in.data(), in.size(), chr_group.data(), chr_group.size(), pair_order.data(), n_groups, &P, out.data(),
                                    out.size(), &n_out);
    const std::string why = rc ? sdf_last_error(ctx) : "";
    sdf_destroy(ctx);
    if (rc == SDF_ERR_INVALID || rc == SDF_ERR_UNSUPPORTED) return ignored(why);
    if (rc) throw "sdf_bucket_merge: " + why;
  }
  int total = 0;
  for (auto &r : read) {
    total += r.second;
    fprintf(log, "\rRead %10d alignments in %s         ", r.second, r.first.c_str());
  }
  fprintf(log, "\nRead total %d alignments\n", total);
  fprintf(log, "\nFinished with sorting\n");
  write_bucket_records(names, out.data(), n_out, nbins, output_dir);
  return true;
}

void bucket_alignments_extern(const std::string &bed_path, int nbins, const std::string &output_dir, bool extend,
                              const std::string &reference, const BucketParams &bp, FILE *log) {
  if (extend && stage_settings().bucket_device &&
      bucket_alignments_records(bed_path, nbins, output_dir, reference, bp, log, 1, stage_settings().device))
    return;
  bucket_alignments_streams(
      [&](const SeedStreamVisitor &visit) {
        for (auto &file : seed_files(bed_path)) {
          std::ifstream fin(file.c_str());
          if (!fin.is_open()) throw "BED file " + bed_path + " does not exist";
          visit(file, fin);
        }
      },
      nbins, output_dir, extend, reference, bp, log);
}

// The host path on seed lines wherever they come from: each_file calls its visitor once per seeds file, in the order the files
// are read, with the file's name and its lines.
void bucket_alignments_streams(const std::function<void(const SeedStreamVisitor &)> &each_file, int nbins, const std::string &output_dir, bool extend,
                               const std::string &reference, const BucketParams &bp, FILE *log) {
  std::map<std::string, int> group_of;
  {
    const auto groups = generate_translation(reference);
    for (int g = 0; g < (int)groups.size(); g++)
      for (auto &name : groups[(size_t)g]) group_of[name] = g;
  }
  // 1. seeds -> extended, side-ordered hits, grouped by the pair of chromosome groups.  The key is the reference's
  //    temporary file name: groups are processed in the order of these strings.
  std::map<std::string, std::vector<std::string>> group_lines;
  int total = 0;
  each_file([&](const std::string &file, std::istream &fin) {
    int count = 0;
    for (std::string line; std::getline(fin, line); count++) {
      Hit h = Hit::from_bed(line);
      if (extend) h.extend(bp.extend_ratio, bp.max_extend);
      order_sides(h);
      const std::string key = output_dir + "/tmp_" + std::to_string(group_of[h.query->name]) + "_" +
                              std::to_string(group_of[h.ref->name]) + ".tmp";
      group_lines[key].push_back(h.to_bed(false));
    }
    total += count;
    fprintf(log, "\rRead %10d alignments in %s         ", count, file.c_str());
  });
  fprintf(log, "\nRead total %d alignments\n", total);

  // 2. merge every group; count the hits per complexity class (sqrt of the area, in thousands)
  int max_complexity = 0;
  std::map<int, int> per_class;
  for (auto &g : group_lines) {
    std::vector<Hit> hits;
    hits.reserve(g.second.size());
    for (auto &line : g.second) hits.push_back(Hit::from_bed(line));
    if (extend) hits = merge_hits(hits, bp.merge_dist);
    g.second.clear();
    for (auto &h : hits) {
      max_complexity = std::max(max_complexity, complexity_of(h));
      per_class[complexity_class(h)]++;
      g.second.push_back(h.to_bed(false));
    }
  }
  fprintf(log, "\nFinished with sorting\n");

  // 3. deal: every complexity class goes round the buckets on its own, starting where the class below it stopped
  //    (src/align_main.cc:147-175), so that each bucket gets its share of cheap and of expensive pairs
  std::vector<int> next_bucket(1, 0);
  for (int c = 1; c <= max_complexity / 1000; c++) next_bucket.push_back((next_bucket[(size_t)c - 1] + per_class[c - 1]) % nbins);
  std::vector<FILE *> out = open_buckets(nbins, output_dir);
  for (auto &g : group_lines)
    for (auto &line : g.second) {
      Hit h = Hit::from_bed(line);
      int &turn = next_bucket[(size_t)complexity_class(h)];
      FILE *f = out[(size_t)turn];
      turn = (turn + 1) % nbins;
      if (h.query->is_rc) {  // the reverse strand belongs on the reference side
        std::swap(h.query, h.ref);
        std::swap(h.query_start, h.ref_start);
        std::swap(h.query_end, h.ref_end);
      }
      fputs(h.to_bed(false).c_str(), f);
      fputs("\n", f);
    }
  for (auto f : out) fclose(f);
}

}  // namespace sdfh
