// `sedef stats diff genome.fa final.bed wgac.tab` (restates reference src/stats_main.cc:397-509, get_differences): how the SDs of
// final.bed and the gold standard's cover the chromosomes, in seven figures on stderr.
//
// The reference paints both files into boost::dynamic_bitset of 250,000,000 bits per chromosome and walks every base of every
// chromosome on the host.  Here the chromosomes final.bed names are uploaded once, as the file has them
// (sdf_pool_append_fasta), and ONE sdf_pool_coverage call does the rest on the device (pool_cover.hip): a chromosome is a region,
// the two sides of a final.bed hit two intervals of set 0 that are partners of each other with min_upper = 100 (the reference's
// `qa < 100 || qb < 100`, :423), the two sides of a WGAC record two intervals of set 1 without a partner.  This file is what is
// left for the host: reading the two tables by the reference's field rules and printing its lines.
// SDF_STATS_DIFF_HOST=1 (StageSettings::stats_diff_host): the same command on sdf_pool_coverage_host, without a device.
//
// Kept from the reference: '#' lines of final.bed are skipped, the others read by from_bed's fields 0-5 and 8-9
// (src/hit.cc:29-63); an end beyond the chromosome is clamped to its length as get_sequence does (src/fasta.cc:105-119); a hit
// with fewer than 100 uppercase bytes -- isupper, so N counts -- on either side is a "miss" and paints nothing; the chromosome
// key is the name alone (the format string at :429-430 has one {} and drops the strand); the first line of wgac.tab is dropped,
// the others read by from_wgac's fields 0, 1, 2, 6, 7, 8 and 16 (src/hit.cc:99-118), skipped when either name is longer than six
// characters or when the record's name was seen before; only chromosomes on which a hit was PAINTED are summed (the reference
// walks its `sedef` map, whose entries are made behind the uppercase test).
//
// Divergences from the reference:
//   * a chromosome SEDEF covers and WGAC never names: the reference's wgac[name] makes an EMPTY bitset there and indexes it out
//     of range; here the WGAC set of such a chromosome is empty.
//   * WGAC coordinates beyond the chromosome's end or below 0: the reference counts such bits up to 250,000,000 and is undefined
//     beyond; here they are clamped to [0, length), and the log says how many records were clamped.  (A WGAC record on a
//     chromosome SEDEF does not cover is never read by the reference's sums either; here it is dropped where it is read.)
//   * chromosomes longer than 250,000,000 bases: undefined in the reference (a set() beyond the bitset), fine here.
//   * the counters are 64 bits wide, not `int`.
//   * a line with too few fields is an error that names the line (the reference asserts); a final.bed start below 0 paints from
//     0 and a start beyond the end paints nothing (the reference sets bits at negative indices, or builds a string of negative
//     length).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <set>

#include "../../../include/sedef_hip.h"
#include "sedef_host.h"

namespace sdfh {

namespace {
struct DiffRegions {  // the chromosomes final.bed names, in the order it names them
  const FastaReference &fr;
  std::map<std::string, int32_t> index;
  std::vector<std::string> names;
  std::vector<int32_t> length;
  explicit DiffRegions(const FastaReference &f) : fr(f) {}
  int32_t of(const std::string &name) {  // (a name the index does not know throws "Chromosome ... does not exist")
    auto it = index.find(name);
    if (it != index.end()) return it->second;
    length.push_back(fr.record(name).entry->length);
    names.push_back(name);
    return index[name] = (int32_t)names.size() - 1;
  }
  int32_t find(const std::string &name) const {
    auto it = index.find(name);
    return it == index.end() ? -1 : it->second;
  }
};

// bases [start, end) of region r as an interval: both ends brought into [0, length]; *clamped: one of them moved
sdf_cover_interval diff_interval(int32_t r, int32_t length, int start, int end, int32_t set, int32_t partner, bool *clamped) {
  const int s = std::min(std::max(start, 0), length), e = std::min(std::max(end, s), length);
  if (clamped) *clamped = s != start || e != end;
  return sdf_cover_interval{r, s, e - s, set, partner, 0};
}
}  // namespace

int stats_diff(const std::string &ref_path, const std::string &bed_path, const std::string &wgac_path, bool host, int device, FILE *log) {
  FastaReference fr(ref_path);
  std::ifstream fin(bed_path.c_str());
  if (!fin.is_open()) throw std::string("BED file ") + bed_path + " does not exist";
  std::ifstream fiw(wgac_path.c_str());
  if (!fiw.is_open()) throw std::string("WGAC file ") + wgac_path + " does not exist";

  DiffRegions regions(fr);
  std::vector<sdf_cover_interval> iv;
  std::string s;
  long long line = 0;
  while (std::getline(fin, s)) {
    ++line;
    if (!s.empty() && s[0] == '#') continue;
    const auto ss = split(s, '\t');
    if (ss.size() < 10) throw "BED line " + std::to_string(line) + " of " + bed_path + " has fewer than 10 fields: " + s;
    const int32_t rq = regions.of(ss[0]), rr = regions.of(ss[3]);
    const int32_t at = (int32_t)iv.size();
    iv.push_back(diff_interval(rq, regions.length[(size_t)rq], atoi(ss[1].c_str()), atoi(ss[2].c_str()), 0, at + 1, nullptr));
    iv.push_back(diff_interval(rr, regions.length[(size_t)rr], atoi(ss[4].c_str()), atoi(ss[5].c_str()), 0, at, nullptr));
  }
  const size_t n_sedef = iv.size();

  // (read before the device call, so that one call paints both sets; its "reading done" line is printed in its place below)
  std::set<std::string> seen;
  long long clamped = 0, elsewhere = 0;
  std::getline(fiw, s);
  line = 1;
  while (std::getline(fiw, s)) {
    ++line;
    const auto ss = split(s, '\t');
    if (ss.size() < 27) throw "WGAC line " + std::to_string(line) + " of " + wgac_path + " has fewer than 27 fields: " + s;
    if (ss[0].size() > 6 || ss[6].size() > 6) continue;
    if (!seen.insert(ss[16]).second) continue;
    const int coords[2][2] = {{atoi(ss[1].c_str()), atoi(ss[2].c_str())}, {atoi(ss[7].c_str()), atoi(ss[8].c_str())}};
    bool moved = false;
    for (int side = 0; side < 2; side++) {
      const int32_t r = regions.find(ss[side ? 6 : 0]);
      if (r < 0) {
        ++elsewhere;
        continue;
      }
      bool c = false;
      iv.push_back(diff_interval(r, regions.length[(size_t)r], coords[side][0], coords[side][1], 1, -1, &c));
      moved |= c;
    }
    clamped += moved;
  }

  const size_t nr = regions.names.size();
  std::vector<sdf_pool_range> ranges(nr);
  std::vector<sdf_cover_counts> counts(nr);
  std::vector<uint8_t> painted(iv.size());
  if (host) {
    std::string pool;
    for (size_t r = 0; r < nr; r++) {
      ranges[r] = sdf_pool_range{(int64_t)pool.size(), regions.length[r], 0};
      pool += fr.get_sequence(regions.names[r]);
    }
    if (sdf_pool_coverage_host(pool.data(), pool.size(), ranges.data(), nr, iv.data(), iv.size(), 100, counts.data(), nullptr, painted.data()) != SDF_OK)
      throw std::string("sdf_pool_coverage_host refused the tables");
  } else {
    sdf_ctx *ctx = sdf_create(device, 0);
    if (!ctx) throw std::string("no usable HIP device: ") + sdf_last_error(nullptr);
    struct Close {
      sdf_ctx *c;
      ~Close() { sdf_destroy(c); }
    } close{ctx};
    for (size_t r = 0; r < nr; r++) {
      const FastaReference::Record rec = fr.record(regions.names[r]);
      int64_t off = 0;
      if (sdf_pool_append_fasta(ctx, rec.bytes, rec.nbytes, rec.entry->length, rec.entry->line_blen, rec.entry->line_len, r == 0, &off) != SDF_OK)
        throw std::string("sdf_pool_append_fasta: ") + sdf_last_error(ctx);
      ranges[r] = sdf_pool_range{off, regions.length[r], 0};
    }
    if (sdf_pool_coverage(ctx, ranges.data(), nr, iv.data(), iv.size(), 100, counts.data(), nullptr, painted.data()) != SDF_OK)
      throw std::string("sdf_pool_coverage: ") + sdf_last_error(ctx);
  }

  long long in = 0, miss = 0;
  std::vector<char> covered(nr, 0);  // the reference's `sedef` map: a chromosome a painted hit names
  for (size_t i = 0; i < n_sedef; i += 2) {
    if (painted[i]) ++in, covered[(size_t)iv[i].region] = covered[(size_t)iv[i + 1].region] = 1;
    else ++miss;
  }
  fprintf(log, "SEDEF reading done (in %lld, miss %lld)!\n", in, miss);
  fprintf(log, "WGAC reading done!\n");
  if (clamped || elsewhere)
    fprintf(log, "[sedef_amd] WGAC: %lld records clamped to their chromosome's length, %lld sides on chromosomes SEDEF does not cover dropped\n",
            clamped, elsewhere);
  sdf_cover_counts t{0, 0, 0, 0, 0, 0, 0};
  for (size_t r = 0; r < nr; r++) {
    if (!covered[r]) continue;
    const sdf_cover_counts &c = counts[r];
    t.a += c.a, t.b += c.b, t.both += c.both, t.a_only += c.a_only, t.b_only += c.b_only;
    t.a_only_upper += c.a_only_upper, t.b_only_upper += c.b_only_upper;
  }
  fprintf(log,
          "SEDEF: spans              %12lld\n"
          "       unique             %12lld\n"
          "       unique (uppercase) %12lld\n"
          "       misses             %12lld\n"
          "       misses (uppercase) %12lld\n"
          "WGAC:  spans              %12lld\n"
          "       intersects         %12lld\n",
          (long long)t.a, (long long)t.a_only, (long long)t.a_only_upper, (long long)t.b_only, (long long)t.b_only_upper, (long long)t.b,
          (long long)t.both);
  return 0;
}

}  // namespace sdfh
