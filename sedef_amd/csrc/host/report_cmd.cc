// `sedef report genome.fa <align dir | *.aligned.bed ...> out_dir` (restates reference sedef.sh:218-229, the block between
// `align generate` and final.bed):
//     cat align/*.aligned.bed | sort -k1,1V -k9,9r -k10,10r -k4,4V -k2,2n -k3,3n -k5,5n -k6,6n | uniq > aligned.bed
//     sedef stats generate genome.fa aligned.bed | sort (same keys) | uniq > final.bed
// Buckets overlap, so one alignment leaves several bucket files; the two sort | uniq passes turn "the output of N buckets" into
// the SD calls.  Here both are ONE sdf_line_order call each (line_order.hip): sdf_line_records parses every line into eight
// ascending keys -- GNU sort's rules under LC_ALL=C taken literally, the field shift of a line with an empty name column
// included (include/sedef_hip.h) --, the device sorts the records by them and orders and compares the lines of equal keys, and
// the lines without SDF_LINE_DUP are written in that order.  Between the two, stats_generate runs on out_dir/aligned.bed as
// `sedef stats generate` runs it; its header line goes through the second ordering like any other line, as in the pipeline.
// SDF_REPORT_HOST=1 (StageSettings::report_host): both orderings by sdf_line_order_host, without a device.  A call in which an
// `n` field has a sign, a decimal point, more than ten digits or a value of 2^32 or more takes the host form as well, said in
// one line on stderr.  Not here: seeds.bed and potentials.bed (plain `cat`s), any locale but C.
#include <dirent.h>
#include <sys/stat.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>

#include "../../../include/sedef_hip.h"
#include "sedef_host.h"

namespace sdfh {

namespace {
struct ReportDevice {  // the context of the two orderings, made when the first of them needs it
  int device;
  sdf_ctx *ctx = nullptr;
  explicit ReportDevice(int d) : device(d) {}
  ~ReportDevice() {
    if (ctx) sdf_destroy(ctx);
  }
  sdf_ctx *get() {
    if (!ctx && !(ctx = sdf_create(device, 0))) throw std::string("no usable HIP device: ") + sdf_last_error(nullptr);
    return ctx;
  }
};

bool ends_with(const std::string &s, const std::string &tail) { return s.size() >= tail.size() && s.compare(s.size() - tail.size(), tail.size(), tail) == 0; }

// the *.aligned.bed files of the inputs: a directory stands for those in it, by name
std::vector<std::string> aligned_files(const std::vector<std::string> &inputs) {
  std::vector<std::string> files;
  for (const std::string &in : inputs) {
    struct stat st;
    if (stat(in.c_str(), &st) != 0) throw in + " does not exist";
    if (!S_ISDIR(st.st_mode)) {
      files.push_back(in);
      continue;
    }
    DIR *d = opendir(in.c_str());
    if (!d) throw std::string("Cannot read directory ") + in;
    std::vector<std::string> found;
    while (const dirent *e = readdir(d))
      if (ends_with(e->d_name, ".aligned.bed")) found.push_back(in + "/" + e->d_name);
    closedir(d);
    std::sort(found.begin(), found.end());
    files.insert(files.end(), found.begin(), found.end());
  }
  return files;
}

// `sort ... | uniq` of `text` to the file `path`; returns the lines written
long long order_to_file(const std::string &text, const std::string &path, const char *what, bool host, ReportDevice &dev, FILE *log) {
  const uint8_t *bytes = (const uint8_t *)text.data();
  size_t pool_bytes = 0, n = 0, kept = 0;
  int plain = 1;
  if (sdf_line_records(bytes, text.size(), nullptr, 0, &pool_bytes, nullptr, 0, &n, nullptr) != SDF_OK)
    throw std::string("report: ") + what + " holds more than 2^30 lines or a line of 4 GiB";
  std::vector<uint8_t> pool(pool_bytes + 16);
  std::vector<sdf_line_rec> lines(n + 1);
  if (sdf_line_records(bytes, text.size(), pool.data(), pool.size(), &pool_bytes, lines.data(), lines.size(), &n, &plain) != SDF_OK)
    throw std::string("report: cannot parse ") + what;
  std::vector<uint32_t> order(n + 1), flags(n + 1);
  if (!host && !plain)
    fprintf(log, "[sedef_amd] report: a number column of %s holds a sign, a decimal point, more than ten digits or a value of 2^32 or more: "
                 "its lines are ordered on the host\n", what);
  if (host || !plain) {
    if (sdf_line_order_host(pool.data(), pool_bytes, lines.data(), n, order.data(), flags.data(), &kept) != SDF_OK)
      throw std::string("sdf_line_order_host refused the lines of ") + what;
  } else if (sdf_line_order(dev.get(), pool.data(), pool_bytes, lines.data(), n, order.data(), flags.data(), &kept) != SDF_OK) {
    throw std::string("sdf_line_order: ") + sdf_last_error(dev.get());
  }
  FILE *fo = fopen(path.c_str(), "w");
  if (!fo) throw std::string("Cannot write ") + path;
  long long written = 0;
  bool ok = true;
  for (size_t p = 0; p < n; p++) {
    if (flags[p] & SDF_LINE_DUP) continue;
    const sdf_line_rec &L = lines[order[p]];
    ok &= fwrite(pool.data() + L.off, 1, L.len, fo) == L.len && fputc('\n', fo) != EOF;
    ++written;
  }
  ok &= fclose(fo) == 0;
  if (!ok) throw std::string("Cannot write ") + path;
  if ((size_t)written != kept) throw std::string("report: the order of ") + what + " counts " + std::to_string(kept) + " lines, " + std::to_string(written) + " were written";
  return written;
}
}  // namespace

int report_command(const std::string &ref_path, const std::vector<std::string> &inputs, const std::string &out_dir, const StatsParams &sp,
                   bool host, int device, FILE *log, long long *counts) {
  const std::vector<std::string> files = aligned_files(inputs);
  if (files.empty()) throw std::string("No *.aligned.bed files in ") + (inputs.empty() ? std::string("the arguments") : inputs[0]);
  std::string text;
  for (const std::string &f : files) {
    std::ifstream in(f.c_str(), std::ios::binary);
    if (!in.is_open()) throw f + " does not exist";
    text.append(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
    if (!text.empty() && text.back() != '\n') text += '\n';  // (a last line without a newline is a line, as for `sort`)
  }
  struct stat st;
  if (stat(out_dir.c_str(), &st) != 0 && mkdir(out_dir.c_str(), 0777) != 0) throw std::string("Cannot create directory ") + out_dir;
  const std::string aligned = out_dir + "/aligned.bed", final_bed = out_dir + "/final.bed";
  ReportDevice dev(device);
  const long long n_aligned = order_to_file(text, aligned, "the aligned buckets", host, dev, log);
  std::string().swap(text);

  char *table = nullptr;
  size_t table_bytes = 0;
  FILE *mem = open_memstream(&table, &table_bytes);
  if (!mem) throw std::string("open_memstream failed");
  struct FreeTable {
    FILE *&f;
    char *&p;
    ~FreeTable() {
      if (f) fclose(f);
      free(p);
    }
  } free_table{mem, table};
  long long stats[3] = {0, 0, 0};
  stats_generate(ref_path, aligned, mem, sp, nullptr, device, stats);
  fclose(mem);
  mem = nullptr;
  const long long n_final = order_to_file(std::string(table, table_bytes), final_bed, "the stats table", host, dev, log);
  fprintf(log, "Report: %lld lines in %s (from %zu files), %lld lines in %s\n", n_aligned, aligned.c_str(), files.size(), n_final, final_bed.c_str());
  if (counts) counts[0] = n_aligned, counts[1] = n_final;
  return 0;
}

}  // namespace sdfh
