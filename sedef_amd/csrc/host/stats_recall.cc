// `sedef stats recall final.bed wgac.tab out.txt` (restates reference scratch/check-overlap.py, the first of the two comparisons
// sedef.sh:253-256 ends with): for every SD of the WGAC gold standard, whether final.bed found it, missed it or covers only
// part of it.
//
// The script is python2 over pandas, a temporary BED file and `bedtools pairtopair -type both`, with a numpy array per base of
// every gold record.  Here both tables become 32-byte records and ONE sdf_pair_recall call on the device (pair_recall.hip)
// answers, per gold row, the found pairs that hit it and the bases of its two sides they cover; bedtools is no part of this
// build, so include/sedef_hip.h's rule IS the project's statement of `pairtopair -type both`: both ends overlap by at least
// one base on equal strands, in either orientation.  This file is what is left for the host: reading the two tables, grouping
// the rows by name and printing the script's lines.  SDF_STATS_RECALL_HOST=1 (StageSettings::stats_recall_host): the same
// command on sdf_pair_recall_host, without a device.  --ignore-strand (StageSettings::stats_recall_ignore_strand):
// SDF_RECALL_IGNORE_STRAND, bedtools' -is.
//
// Kept from the script: the first line of wgac.tab is its header; a row is read by the fields Hit::from_wgac reads (src/hit.cc:
// 99-118: 0-2, 5, 6-8, and 16 for the name), skipped when either chromosome name holds a '_' (:35), its strands '+' and -- when
// field 5 is '_' -- '-' (:39); '#' lines of final.bed are skipped, the others read by from_bed's fields 0-5 and 8-9; rows are
// grouped by name (WGAC lists a pair once per orientation under one name), "WGAC:" counts names and all data lines (:43); a
// name no row of which is hit is MISSED and printed with the coordinates of its LAST row (name_to_coor is overwritten, :42), the
// MISS lines sorted by name (:99-106); a name is PARTIAL when round(p * 100) < 80 on either side -- python2's round, C's
// round() --, the PART lines sorted by p1 + p2 (:141-144); every format string is the script's, thousands separators included.
//
// Divergences from the script:
//   * ties among PART lines are ordered by name; the script's order there is python2's dict order.
//   * a name's coverage comes from ONE row -- the first in file order that has a hit -- and that row's own hits, painted for both
//     orientations.  The script sizes its arrays by one row (h[0][1]) and paints every row's hits into them through offsets of
//     another row; it also paints direct overlaps only, so a pair found in the other orientation counts as covered 0%.
//   * touching ends paint nothing here; they paint nothing in the script either (an empty slice), but its `<=` lets them through.
//   * a row with an empty side is skipped and counted on stderr; the script divides by zero there.
//   * the counters are 64 bits wide.
//   * a line with too few fields, a start below 0 or a start behind its end is an error that names the line.
//   * without a single name the three percentages print as 0.0; the script divides by zero.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>

#include "../../../include/sedef_hip.h"
#include "sedef_host.h"

namespace sdfh {

namespace {
// python's "{:,}" of an integer
std::string with_commas(long long v) {
  std::string digits = std::to_string(v < 0 ? -v : v), out;
  for (size_t i = 0; i < digits.size(); i++) {
    if (i && (digits.size() - i) % 3 == 0) out += ',';
    out += digits[i];
  }
  return v < 0 ? "-" + out : out;
}

struct RecallChroms {  // one table over both files, in order of first appearance
  std::map<std::string, int32_t> index;
  int32_t of(const std::string &name) {
    auto it = index.find(name);
    if (it != index.end()) return it->second;
    const int32_t id = (int32_t)index.size();
    return index[name] = id;
  }
};

struct GoldRow {
  std::string chr1, chr2, strand;  // as the file has them
  int start1, end1, start2, end2;
};
struct GoldName {
  std::vector<size_t> rows;  // indices into the gold records, in file order
};

void check_side(const char *what, long long line, const std::string &path, int start, int end, const std::string &s) {
  if (start < 0 || start > end)
    throw std::string(what) + " line " + std::to_string(line) + " of " + path + " has a start below 0 or behind its end: " + s;
}
}  // namespace

int stats_recall(const std::string &bed_path, const std::string &wgac_path, const std::string &out_path, bool host, bool ignore_strand,
                 int device, FILE *report, FILE *log) {
  std::ifstream fin(bed_path.c_str());
  if (!fin.is_open()) throw std::string("BED file ") + bed_path + " does not exist";
  std::ifstream fiw(wgac_path.c_str());
  if (!fiw.is_open()) throw std::string("WGAC file ") + wgac_path + " does not exist";

  RecallChroms chroms;
  std::vector<sdf_pair_rec> found, gold;
  std::string s;
  long long line = 0;
  while (std::getline(fin, s)) {
    ++line;
    if (!s.empty() && s[0] == '#') continue;
    const auto ss = split(s, '\t');
    if (ss.size() < 10) throw "BED line " + std::to_string(line) + " of " + bed_path + " has fewer than 10 fields: " + s;
    const int c[4] = {atoi(ss[1].c_str()), atoi(ss[2].c_str()), atoi(ss[4].c_str()), atoi(ss[5].c_str())};
    check_side("BED", line, bed_path, c[0], c[1], s);
    check_side("BED", line, bed_path, c[2], c[3], s);
    const uint32_t strands = (ss[8].empty() || ss[8][0] != '+' ? 1u : 0u) | (ss[9].empty() || ss[9][0] != '+' ? 2u : 0u);
    found.push_back(sdf_pair_rec{chroms.of(ss[0]), c[0], c[1], chroms.of(ss[3]), c[2], c[3], strands, 0u});
  }

  std::vector<GoldRow> rows;               // one per gold record
  std::map<std::string, GoldName> names;  // (sorted by name: the MISS lines' order)
  long long data_lines = 0, empty_sides = 0;
  std::getline(fiw, s);
  line = 1;
  while (std::getline(fiw, s)) {
    ++line;
    const auto ss = split(s, '\t');
    if (ss.size() < 17) throw "WGAC line " + std::to_string(line) + " of " + wgac_path + " has fewer than 17 fields: " + s;
    ++data_lines;
    if (ss[0].find('_') != std::string::npos || ss[6].find('_') != std::string::npos) continue;
    GoldRow r{ss[0], ss[6], ss[5], atoi(ss[1].c_str()), atoi(ss[2].c_str()), atoi(ss[7].c_str()), atoi(ss[8].c_str())};
    check_side("WGAC", line, wgac_path, r.start1, r.end1, s);
    check_side("WGAC", line, wgac_path, r.start2, r.end2, s);
    if (r.start1 == r.end1 || r.start2 == r.end2) {
      ++empty_sides;
      continue;
    }
    names[ss[16]].rows.push_back(gold.size());
    gold.push_back(sdf_pair_rec{chroms.of(r.chr1), r.start1, r.end1, chroms.of(r.chr2), r.start2, r.end2, r.strand == "_" ? 2u : 0u, 0u});
    rows.push_back(r);
  }
  if (empty_sides) fprintf(log, "[sedef_amd] WGAC: %lld rows with an empty side skipped\n", empty_sides);

  std::vector<sdf_pair_recall_rec> rec(gold.size());
  const uint32_t flags = ignore_strand ? SDF_RECALL_IGNORE_STRAND : 0u;
  if (host) {
    if (sdf_pair_recall_host(gold.data(), gold.size(), found.data(), found.size(), flags, rec.data()) != SDF_OK)
      throw std::string("sdf_pair_recall_host refused the tables");
  } else {
    sdf_ctx *ctx = sdf_create(device, 0);
    if (!ctx) throw std::string("no usable HIP device: ") + sdf_last_error(nullptr);
    struct Close {
      sdf_ctx *c;
      ~Close() { sdf_destroy(c); }
    } close{ctx};
    if (sdf_pair_recall(ctx, gold.data(), gold.size(), found.data(), found.size(), flags, rec.data()) != SDF_OK)
      throw std::string("sdf_pair_recall: ") + sdf_last_error(ctx);
  }

  FILE *fo = fopen(out_path.c_str(), "w");
  if (!fo) throw std::string("Cannot write ") + out_path;
  struct CloseFile {
    FILE *f;
    ~CloseFile() { fclose(f); }
  } close_fo{fo};
  struct Part {
    double p1, p2;
    const std::string *name;
  };
  std::vector<Part> partial;
  long long missed = 0, full = 0;
  for (const auto &kv : names) {
    const std::vector<size_t> &of = kv.second.rows;
    const auto hit = std::find_if(of.begin(), of.end(), [&](size_t g) { return rec[g].n_hits != 0; });
    if (hit == of.end()) {
      ++missed;
      const GoldRow &r = rows[of.back()];
      fprintf(fo, "MISS\t%s\t%d\t%d\t%s\t%d\t%d\t%s\tlen1=%s\tlen2=%s\thttp://humanparalogy.gs.washington.edu/build37/%s\n", r.chr1.c_str(),
              r.start1, r.end1, r.chr2.c_str(), r.start2, r.end2, r.strand.c_str(), with_commas((long long)r.end1 - r.start1).c_str(),
              with_commas((long long)r.end2 - r.start2).c_str(), kv.first.c_str());
      continue;
    }
    const GoldRow &r = rows[*hit];
    const double p1 = (double)rec[*hit].cov1 / (double)(r.end1 - r.start1), p2 = (double)rec[*hit].cov2 / (double)(r.end2 - r.start2);
    if (std::round(p1 * 100) < 80 || std::round(p2 * 100) < 80) partial.push_back(Part{p1, p2, &kv.first});
    else ++full;
  }
  std::stable_sort(partial.begin(), partial.end(), [](const Part &a, const Part &b) { return a.p1 + a.p2 < b.p1 + b.p2; });  // (names ascend already)
  for (const Part &p : partial)
    fprintf(fo, "PART\t%.2f\t%.2f\thttp://humanparalogy.gs.washington.edu/build37/%s\n", p.p1 * 100, p.p2 * 100, p.name->c_str());

  const long long n_names = (long long)names.size();
  const auto pct = [&](long long v) { return n_names ? 100.0 * (double)v / (double)n_names : 0.0; };
  fprintf(report, "WGAC:     %6s (%s lines)\n", with_commas(n_names).c_str(), with_commas(data_lines).c_str());
  fprintf(report, "Missed:  %7s hits (%4.1f%%)\n", with_commas(missed).c_str(), pct(missed));
  fprintf(report, "Partial: %7s hits (%4.1f%%)\n", with_commas((long long)partial.size()).c_str(), pct((long long)partial.size()));
  fprintf(report, "Full:    %7s hits (%4.1f%%)\n", with_commas(full).c_str(), pct(full));
  return 0;
}

}  // namespace sdfh
