// The C ABI: line order (include/sedef_hip.h states the contract; line_order.hip holds the kernels; what a line must be is
// sdf_kernels.h's line_rec_bad) -- the `_host` form, the form over host arrays and the device form over one chain of launches.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstring>
#include <string>
#include <string_view>
#include <unordered_map>
#include <vector>

#include "sdf_entry.h"

using namespace sdf;

namespace {
constexpr size_t kLineMaxN = (size_t)1 << 30, kLineMaxPool = (size_t)1 << 40;

// what every form asks of its scalars; the pointers are the caller's arrays wherever they lie
int check_lines_scalars(const void *pool, size_t pool_bytes, const void *lines, size_t n, const void *order, const void *flags, const char **why) {
  if (n > kLineMaxN || pool_bytes >= kLineMaxPool) return *why = "more than 2^30 lines or a pool of 2^40 bytes or more in one call", SDF_ERR_UNSUPPORTED;
  if ((n && (!lines || !order || !flags)) || (pool_bytes && !pool)) return *why = "invalid arguments", SDF_ERR_INVALID;
  return SDF_OK;
}
// ... and, where the arrays are the host's, of every line
int check_lines(const uint8_t *pool, size_t pool_bytes, const sdf_line_rec *lines, size_t n, const void *order, const void *flags,
                const size_t *n_kept, std::string *why) {
  const char *w = "";
  if (int rc = check_lines_scalars(pool, pool_bytes, lines, n, order, flags, &w)) return *why = w, rc;
  if (!n_kept) return *why = "invalid arguments", SDF_ERR_INVALID;
  for (size_t i = 0; i < n; i++)
    if (line_rec_bad(lines[i], pool_bytes))
      return *why = "line " + std::to_string(i) + ": off is no multiple of 16, reserved != 0 or the range runs past the pool", SDF_ERR_INVALID;
  return SDF_OK;
}

// the order inside a run: memcmp over the common length, the shorter line first, identical lines by index
struct LineLess {
  const uint8_t *pool;
  const sdf_line_rec *lines;
  int compare(uint32_t a, uint32_t b) const {
    const sdf_line_rec &A = lines[a], &B = lines[b];
    const uint32_t common = std::min(A.len, B.len);
    const int c = common ? memcmp(pool + A.off, pool + B.off, common) : 0;
    return c ? c : A.len < B.len ? -1 : A.len > B.len ? 1 : 0;
  }
  bool operator()(uint32_t a, uint32_t b) const {
    const int c = compare(a, b);
    return c ? c < 0 : a < b;
  }
};

// Places [lo, hi) hold a run in index order: ordered where they lie, SDF_LINE_DUP where a line equals the one in front of it,
// SDF_LINE_WIDE on all of a run of more than kLineRun.  Returns the duplicates.
size_t line_run_host(const LineLess &less, uint32_t *order, uint32_t *flags, size_t lo, size_t hi) {
  std::sort(order + lo, order + hi, less);
  const uint32_t wide = hi - lo > (size_t)kLineRun ? SDF_LINE_WIDE : 0u;
  size_t dups = 0;
  for (size_t p = lo; p < hi; p++) {
    const bool dup = p > lo && less.compare(order[p - 1], order[p]) == 0;
    flags[p] = wide | (dup ? SDF_LINE_DUP : 0u);
    dups += dup;
  }
  return dups;
}

// ---- the parse: GNU sort's fields and comparisons under LC_ALL=C, restated (include/sedef_hip.h: sdf_line_records) ----------
using Text = std::string_view;
inline bool line_blank(char c) { return c == ' ' || c == '\t'; }
inline bool line_digit(char c) { return c >= '0' && c <= '9'; }
inline bool line_alpha(char c) { return (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z'); }

// field k (from 1) of a line without -t: behind k - 1 groups of blanks-then-non-blanks, up to the end of the k-th; its leading
// blanks are part of it
Text line_field(Text s, int k) {
  size_t at = 0, begin = 0;
  for (int f = 0; f < k; f++) {
    begin = at;
    while (at < s.size() && line_blank(s[at])) at++;
    while (at < s.size() && !line_blank(s[at])) at++;
  }
  return s.substr(begin, at - begin);
}

// version order.  A character of a non-digit run: '~' in front of the end of the string, the end (and a digit, which ends the
// run) in front of the letters, every other byte behind them.
inline int ver_class(unsigned char c) { return line_digit((char)c) ? 0 : line_alpha((char)c) ? c : c == '~' ? -1 : c + 256; }
int ver_body(Text a, Text b) {
  size_t i = 0, j = 0;
  while (i < a.size() || j < b.size()) {
    while ((i < a.size() && !line_digit(a[i])) || (j < b.size() && !line_digit(b[j]))) {
      const int x = i < a.size() ? ver_class((unsigned char)a[i]) : 0, y = j < b.size() ? ver_class((unsigned char)b[j]) : 0;
      if (x != y) return x < y ? -1 : 1;
      i++, j++;
    }
    while (i < a.size() && a[i] == '0') i++;
    while (j < b.size() && b[j] == '0') j++;
    const size_t da = i, db = j;
    while (i < a.size() && line_digit(a[i])) i++;
    while (j < b.size() && line_digit(b[j])) j++;
    if (i - da != j - db) return i - da < j - db ? -1 : 1;  // (no leading zeros: the longer run is the larger number)
    if (const int c = a.compare(da, i - da, b, db, j - db)) return c < 0 ? -1 : 1;
  }
  return 0;
}
// where the file suffix (\.[A-Za-z~][A-Za-z0-9~]*)*$ of s starts
size_t ver_suffix(Text s) {
  size_t end = s.size();
  for (;;) {
    size_t at = end;
    while (at > 0 && (line_alpha(s[at - 1]) || line_digit(s[at - 1]) || s[at - 1] == '~')) at--;
    if (at == 0 || s[at - 1] != '.' || at == end || line_digit(s[at])) return end;
    end = at - 1;
  }
}
int ver_compare(Text a, Text b) {
  const int simple = a.compare(b);
  if (simple == 0) return 0;
  if (a.empty() || b.empty()) return a.empty() ? -1 : 1;
  for (const char *first : {".", ".."}) {
    if (a == first) return -1;
    if (b == first) return 1;
  }
  if ((a[0] == '.') != (b[0] == '.')) return a[0] == '.' ? -1 : 1;
  if (a[0] == '.') a.remove_prefix(1), b.remove_prefix(1);
  const Text ca = a.substr(0, ver_suffix(a)), cb = b.substr(0, ver_suffix(b));
  const int r = ca == cb ? ver_body(a, b) : ver_body(ca, cb);  // (equal without their suffixes: with them)
  return r ? r : simple < 0 ? -1 : 1;
}

// the number in front of an n field: sign, digits in front of the point without leading zeros, digits behind it without trailing ones
struct LineNumber {
  bool neg = false, plain = true;  // plain: no sign, no point, at most ten digits, below 2^32
  Text whole, frac;
  uint32_t value = 0;
};
LineNumber line_number(Text f) {
  LineNumber N;
  size_t at = 0;
  while (at < f.size() && line_blank(f[at])) at++;
  if (at < f.size() && (f[at] == '-' || f[at] == '.')) N.plain = false;
  if (at < f.size() && f[at] == '-') N.neg = true, at++;
  size_t d0 = at;
  while (at < f.size() && line_digit(f[at])) at++;
  const size_t n_digits = at - d0;
  while (d0 < at && f[d0] == '0') d0++;
  N.whole = f.substr(d0, at - d0);
  if (at < f.size() && f[at] == '.') {
    N.plain = false;
    size_t e = ++at;
    while (e < f.size() && line_digit(f[e])) e++;
    while (e > at && f[e - 1] == '0') e--;
    N.frac = f.substr(at, e - at);
  }
  if (N.whole.empty() && N.frac.empty()) N.neg = false;  // (-0 is 0)
  unsigned long long v = 0;
  if (n_digits > 10) N.plain = false;
  else
    for (char c : N.whole) v = v * 10 + (unsigned long long)(c - '0');
  if (v >> 32) N.plain = false;
  N.value = (uint32_t)v;
  return N;
}
inline int line_number_compare(const LineNumber &a, const LineNumber &b) {
  if (a.neg != b.neg) return a.neg ? -1 : 1;
  int c = a.whole.size() != b.whole.size() ? (a.whole.size() < b.whole.size() ? -1 : 1) : a.whole.compare(b.whole);
  if (c == 0) c = a.frac.compare(b.frac);
  c = c < 0 ? -1 : c > 0 ? 1 : 0;
  return a.neg ? -c : c;
}

// ranks[i] = the rank of items[i] among the distinct items by `cmp` (items that compare 0 share a rank); returns the number of
// ranks.  Only the distinct texts are sorted -- a few dozen chromosome names and strands among any number of lines.
template <class Cmp>
uint32_t line_ranks(const std::vector<Text> &items, Cmp cmp, std::vector<uint32_t> *ranks) {
  std::unordered_map<Text, uint32_t> id_of;
  std::vector<Text> distinct;
  std::vector<uint32_t> id(items.size());
  for (size_t i = 0; i < items.size(); i++) {
    const auto at = id_of.emplace(items[i], (uint32_t)distinct.size());
    if (at.second) distinct.push_back(items[i]);
    id[i] = at.first->second;
  }
  std::vector<uint32_t> by(distinct.size()), rank_of(distinct.size());
  for (size_t d = 0; d < by.size(); d++) by[d] = (uint32_t)d;
  std::sort(by.begin(), by.end(), [&](uint32_t x, uint32_t y) { return cmp(distinct[x], distinct[y]) < 0; });
  uint32_t rank = 0;
  for (size_t p = 0; p < by.size(); p++) {
    if (p && cmp(distinct[by[p - 1]], distinct[by[p]]) != 0) rank++;
    rank_of[by[p]] = rank;
  }
  ranks->resize(items.size());
  for (size_t i = 0; i < items.size(); i++) (*ranks)[i] = rank_of[id[i]];
  return by.empty() ? 0u : rank + 1u;
}

// The launches of a call on `st`, nothing read back: d_counts as include/sedef_hip.h has them.
int lines_launch(sdf_ctx *ctx, const uint8_t *d_pool, size_t pool_bytes, const sdf_line_rec *d_lines, size_t n, uint32_t *d_order,
                 uint32_t *d_flags, uint32_t *d_counts, hipStream_t st) {
  // the workspace, in pieces of whole 256 bytes: the count of listed runs, the sort's keys and places twice, the head bytes, the list
  size_t at = 0;
  const auto piece = [&](size_t bytes) {
    const size_t off = at;
    at += (bytes + 255) & ~(size_t)255;
    return off;
  };
  const size_t o_runs = piece(sizeof(uint32_t)), o_key_a = piece(n * 8), o_key_b = piece(n * 8), o_val_a = piece(n * 4), o_val_b = piece(n * 4),
               o_head = piece(n), o_list = piece((n / 2 + 1) * 4);
  SDF_HIP(ctx->lo_ws.reserve(at));
  char *ws = (char *)ctx->lo_ws.p;
  uint32_t *n_runs = (uint32_t *)(ws + o_runs), *val_a = (uint32_t *)(ws + o_val_a), *val_b = (uint32_t *)(ws + o_val_b),
           *list = (uint32_t *)(ws + o_list);
  unsigned long long *key_a = (unsigned long long *)(ws + o_key_a), *key_b = (unsigned long long *)(ws + o_key_b);
  uint8_t *head = (uint8_t *)(ws + o_head);
  size_t tmp = 0;
  SDF_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp, key_a, key_b, val_a, val_b, (int)n, 0, 64, st));
  tmp += 256;
  SDF_HIP(ctx->lo_tmp.reserve(tmp));
  SDF_HIP(hipMemsetAsync(n_runs, 0, sizeof(uint32_t), st));  // (every call's own: nothing of the call before is read)
  SDF_HIP(hipMemsetAsync(d_counts, 0, 3 * sizeof(uint32_t), st));
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  // four stable passes, least significant pair of keys first; the places go val_a -> val_b -> val_a -> val_b -> d_order
  for (int pair = 3; pair >= 0; pair--) {
    const uint32_t *from = pair == 3 ? nullptr : (pair & 1) ? val_a : val_b;
    uint32_t *in = (pair & 1) ? val_a : val_b, *out = pair == 0 ? d_order : (pair & 1) ? val_b : val_a;
    hipLaunchKernelGGL(line_keys_kernel, grid, block, 0, st, d_lines, from, in, key_a, (int)n, pair, (unsigned long long)pool_bytes, d_counts);
    SDF_HIP(hipcub::DeviceRadixSort::SortPairs(ctx->lo_tmp.p, tmp, key_a, key_b, in, out, (int)n, 0, 64, st));
    ctx->launches += 1;
  }
  hipLaunchKernelGGL(line_heads_kernel, grid, block, 0, st, d_lines, (const uint32_t *)d_order, (int)n, head, d_flags, list, n_runs, d_counts);
  // (a fixed grid, sixteen wavefronts a CU of 256: the kernel strides over the listed runs, whose number only the device knows)
  const size_t tie_grid = std::min(n / 2 + 1, (size_t)4096);
  hipLaunchKernelGGL(line_tie_kernel, dim3((unsigned)tie_grid), dim3(64), 0, st, d_pool, (unsigned long long)pool_bytes, d_lines, (int)n,
                     (const uint8_t *)head, (const uint32_t *)list, (const uint32_t *)n_runs, d_order, d_flags, d_counts);
  ctx->launches += 2;
  SDF_HIP(hipGetLastError());
  return SDF_OK;
}
}  // namespace

extern "C" int sdf_line_order_device(sdf_ctx *ctx, const uint8_t *d_pool, size_t pool_bytes, const sdf_line_rec *d_lines, size_t n,
                                     uint32_t *d_order, uint32_t *d_flags, uint32_t *d_counts, void *stream) {
  if (!ctx) return SDF_ERR_INVALID;
  ctx->err.clear();
  const char *why = "";
  if (int rc = check_lines_scalars(d_pool, pool_bytes, d_lines, n, d_order, d_flags, &why))
    return refuse(ctx, rc, std::string("sdf_line_order_device: ") + why);
  if (!d_counts) return refuse(ctx, SDF_ERR_INVALID, "sdf_line_order_device: invalid arguments");
  if ((uintptr_t)d_pool & 15) return refuse(ctx, SDF_ERR_INVALID, "sdf_line_order_device: the pool must start at a multiple of 16 bytes");
  SDF_HIP(hipSetDevice(ctx->device));
  hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
  if (n == 0) {
    SDF_HIP(hipMemsetAsync(d_counts, 0, 3 * sizeof(uint32_t), st));
    return SDF_OK;
  }
  return lines_launch(ctx, d_pool, pool_bytes, d_lines, n, d_order, d_flags, d_counts, st);
}

extern "C" int sdf_line_order(sdf_ctx *ctx, const uint8_t *pool, size_t pool_bytes, const sdf_line_rec *lines, size_t n, uint32_t *order,
                              uint32_t *flags, size_t *n_kept) {
  if (!ctx) return SDF_ERR_INVALID;
  ctx->err.clear();
  std::string why;
  if (int rc = check_lines(pool, pool_bytes, lines, n, order, flags, n_kept, &why)) return refuse(ctx, rc, "sdf_line_order: " + why);
  *n_kept = 0;
  if (n == 0) return SDF_OK;
  SDF_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  for (DevBuf *b : {&ctx->lo_ws, &ctx->lo_tmp, &ctx->lo_pool, &ctx->lo_lines, &ctx->lo_out}) b->new_call();
  SDF_HIP(ctx->lo_out.reserve(256 + 2 * n * sizeof(uint32_t)));
  SDF_HIP(ctx->lo_pool.reserve(std::max(pool_bytes, (size_t)16)));  // (a pool of no bytes still gives the kernels a pointer)
  if (int rc = upload_all(ctx, st, {{ctx->lo_pool, pool, pool_bytes}, {ctx->lo_lines, lines, n * sizeof(sdf_line_rec)}})) return rc;
  uint32_t *d_counts = (uint32_t *)ctx->lo_out.p, *d_order = (uint32_t *)((char *)ctx->lo_out.p + 256), *d_flags = d_order + n;
  if (int rc = lines_launch(ctx, (const uint8_t *)ctx->lo_pool.p, pool_bytes, (const sdf_line_rec *)ctx->lo_lines.p, n, d_order, d_flags, d_counts, st))
    return rc;
  uint32_t counts[3] = {0, 0, 0};
  SDF_HIP(hipMemcpyAsync(counts, d_counts, sizeof counts, hipMemcpyDeviceToHost, st));
  SDF_HIP(hipMemcpyAsync(order, d_order, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  SDF_HIP(hipMemcpyAsync(flags, d_flags, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  SDF_HIP(hipStreamSynchronize(st));
  if (counts[2] != 0)  // (the host's check passed every line: the two disagree)
    return refuse(ctx, SDF_ERR_INVALID, "sdf_line_order: the device refused " + std::to_string(counts[2]) + " lines the host's check passed");
  // the runs the tie kernel does not take: the same order on the host.  (Two WIDE runs may touch: the keys part them.)
  size_t kept = counts[0];
  const LineLess less{pool, lines};
  for (size_t p = 0; counts[1] != 0 && p < n;) {
    if (!(flags[p] & SDF_LINE_WIDE)) {
      p++;
      continue;
    }
    size_t hi = p + 1;
    while (hi < n && (flags[hi] & SDF_LINE_WIDE) && line_keys_equal(lines[order[p]], lines[order[hi]])) hi++;
    kept -= line_run_host(less, order, flags, p, hi);
    p = hi;
  }
  *n_kept = kept;
  return SDF_OK;
}

extern "C" int sdf_line_order_host(const uint8_t *pool, size_t pool_bytes, const sdf_line_rec *lines, size_t n, uint32_t *order, uint32_t *flags,
                                   size_t *n_kept) {
  std::string why;
  if (int rc = check_lines(pool, pool_bytes, lines, n, order, flags, n_kept, &why)) return rc;
  for (size_t i = 0; i < n; i++) order[i] = (uint32_t)i;
  // by the keys, stable; then every run by its bytes
  std::stable_sort(order, order + n, [&](uint32_t a, uint32_t b) {
    return std::lexicographical_compare(lines[a].key, lines[a].key + 8, lines[b].key, lines[b].key + 8);
  });
  const LineLess less{pool, lines};
  size_t kept = n;
  for (size_t p = 0; p < n;) {
    size_t hi = p + 1;
    while (hi < n && line_keys_equal(lines[order[p]], lines[order[hi]])) hi++;
    kept -= line_run_host(less, order, flags, p, hi);
    p = hi;
  }
  *n_kept = kept;
  return SDF_OK;
}

extern "C" int sdf_line_records(const uint8_t *text, size_t text_bytes, uint8_t *pool, size_t pool_cap, size_t *pool_bytes, sdf_line_rec *lines,
                                size_t lines_cap, size_t *n, int *plain) {
  if (!pool_bytes || !n || (text_bytes && !text)) return SDF_ERR_INVALID;
  // the lines, and where each goes
  std::vector<Text> line;
  for (size_t at = 0; at < text_bytes;) {
    const void *nl = memchr(text + at, '\n', text_bytes - at);
    const size_t end = nl ? (size_t)((const uint8_t *)nl - text) : text_bytes;
    if (end - at >= ((size_t)1 << 32) || line.size() >= kLineMaxN) return SDF_ERR_UNSUPPORTED;
    line.emplace_back((const char *)text + at, end - at);
    at = end + 1;
  }
  size_t need = 0;
  for (const Text &s : line) need += (s.size() + 15) & ~(size_t)15;
  *pool_bytes = need;
  *n = line.size();
  if (!pool || !lines) return SDF_OK;
  if (pool_cap < need || lines_cap < line.size()) return SDF_ERR_INVALID;
  const size_t count = line.size();
  // the eight fields in key order, then their ranks or values
  static const int kField[8] = {1, 9, 10, 4, 2, 3, 5, 6};
  std::vector<Text> field[8];
  for (int k = 0; k < 8; k++) {
    field[k].resize(count);
    for (size_t i = 0; i < count; i++) field[k][i] = line_field(line[i], kField[k]);
  }
  std::vector<uint32_t> key[8];
  for (int k : {0, 3}) line_ranks(field[k], ver_compare, &key[k]);
  for (int k : {1, 2}) {
    const uint32_t distinct = line_ranks(field[k], [](Text a, Text b) { return a.compare(b); }, &key[k]);
    for (uint32_t &r : key[k]) r = distinct - 1u - r;
  }
  bool all_plain = true;
  for (int k = 4; k < 8; k++) {
    key[k].resize(count);
    for (size_t i = 0; i < count; i++) {
      const LineNumber N = line_number(field[k][i]);
      all_plain &= N.plain;
      key[k][i] = N.value;
    }
  }
  if (!all_plain)  // (ranks by numeric comparison: fields that read as the same number share one)
    for (int k = 4; k < 8; k++) line_ranks(field[k], [](Text a, Text b) { return line_number_compare(line_number(a), line_number(b)); }, &key[k]);
  if (plain) *plain = all_plain ? 1 : 0;
  size_t off = 0;
  for (size_t i = 0; i < count; i++) {
    const size_t room = (line[i].size() + 15) & ~(size_t)15;
    if (!line[i].empty()) memcpy(pool + off, line[i].data(), line[i].size());
    memset(pool + off + line[i].size(), 0, room - line[i].size());
    lines[i] = sdf_line_rec{(uint64_t)off, (uint32_t)line[i].size(), 0u, {key[0][i], key[1][i], key[2][i], key[3][i], key[4][i], key[5][i], key[6][i], key[7][i]}};
    off += room;
  }
  return SDF_OK;
}
