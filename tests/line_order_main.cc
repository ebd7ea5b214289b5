// sdf_line_records and sdf_line_order_host (sedef_amd/csrc/sdf_report_api.hip) in a program of its own, against the order
// written out here -- the eight keys, then the bytes, the shorter line first, duplicates by comparison with the line in front --
// on generated lines of `align generate`'s shape with and without a name column, in pools of exact size: built with
// -fsanitize=address,undefined on the host side and run by tests/test_line_order_cpu.py, on the CPU.  Exit status 0 and
// "line order ok" when every statement holds; a finding makes the sanitizer's runtime end the program itself.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../include/sedef_hip.h"

#define CHECK(cond)                                               \
  do {                                                            \
    if (!(cond)) {                                                \
      fprintf(stderr, "line %d: %s fails\n", __LINE__, #cond);    \
      return 1;                                                   \
    }                                                             \
  } while (0)

int main() {
  std::mt19937 rng(11);
  const auto upto = [&](int n) { return (int)(rng() % (unsigned)n); };
  const char *chroms[] = {"chr1", "chr2", "chr10", "chrX", "chr1_gl000191_random"};
  for (int draw = 0; draw < 40; draw++) {
    const int n = draw == 0 ? 0 : draw == 1 ? 1 : draw == 3 ? 400 : 1 + upto(400);
    std::vector<std::string> line;
    for (int i = 0; i < n; i++) {
      if (!line.empty() && upto(3) == 0) {
        line.push_back(line[(size_t)upto((int)line.size())]);
        continue;
      }
      std::string s = std::string(chroms[upto(5)]) + "\t" + std::to_string(upto(6)) + "\t" + std::to_string(10 + upto(3)) + "\t" + chroms[upto(5)] + "\t" +
                      std::to_string(upto(3)) + "\t" + std::to_string(upto(3)) + "\t" + (upto(2) ? "S" : "") + "\t0.0\t" + (upto(2) ? "+" : "-") + "\t" +
                      (upto(2) ? "+" : "-") + "\t" + std::to_string(upto(3)) + "\t" + std::string((size_t)upto(draw == 2 ? 3000 : 40), "MX"[upto(2)]);
      if (draw == 3 && upto(2) == 0) s = std::string(chroms[0]) + "\t1\t10\t" + chroms[1] + "\t1\t1\tS\t0.0\t+\t+\t" + std::string((size_t)upto(90), 'M');  // a run beyond 64
      line.push_back(s);
    }
    std::string text;
    for (const std::string &s : line) text += s + "\n";
    size_t pool_bytes = 0, count = 0;
    int plain = 0;
    CHECK(sdf_line_records((const uint8_t *)text.data(), text.size(), nullptr, 0, &pool_bytes, nullptr, 0, &count, nullptr) == SDF_OK);
    CHECK(count == (size_t)n);
    std::vector<uint8_t> pool(pool_bytes ? pool_bytes : 1);  // (exact sizes: a read or a write beyond them is a finding)
    std::vector<sdf_line_rec> recs(count ? count : 1);
    CHECK(sdf_line_records((const uint8_t *)text.data(), text.size(), pool.data(), pool_bytes, &pool_bytes, recs.data(), count, &count, &plain) == SDF_OK);
    CHECK(plain == 1);
    std::vector<uint32_t> order(count ? count : 1), flags(count ? count : 1);
    size_t kept = ~(size_t)0;
    CHECK(sdf_line_order_host(pool.data(), pool_bytes, recs.data(), count, order.data(), flags.data(), &kept) == SDF_OK);
    // the definition: a permutation, ascending by (keys, bytes, index); DUP exactly where the line equals the one in front
    std::vector<char> seen(count, 0);
    size_t dups = 0, wide = 0;
    for (size_t p = 0; p < count; p++) {
      CHECK(order[p] < count && !seen[order[p]]);
      seen[order[p]] = 1;
      const sdf_line_rec &B = recs[order[p]];
      CHECK(B.off % 16 == 0 && B.len == line[order[p]].size() && memcmp(pool.data() + B.off, line[order[p]].data(), B.len) == 0);
      if (p == 0) {
        CHECK(!(flags[0] & SDF_LINE_DUP));
        continue;
      }
      const sdf_line_rec &A = recs[order[p - 1]];
      const bool keys_less = std::lexicographical_compare(A.key, A.key + 8, B.key, B.key + 8), keys_same = std::equal(A.key, A.key + 8, B.key);
      CHECK(keys_less || keys_same);
      const std::string &a = line[order[p - 1]], &b = line[order[p]];
      if (keys_same) CHECK(a < b || (a == b && order[p - 1] < order[p]));
      CHECK(((flags[p] & SDF_LINE_DUP) != 0) == (a == b));
      dups += a == b;
      wide += (flags[p] & SDF_LINE_WIDE) != 0;
    }
    CHECK(kept == count - dups);
    if (draw == 3) CHECK(wide > 64);
    else CHECK(wide == 0);
  }
  // the parse: the field shift of an empty name column, a missing field, the number columns the records do not take
  {
    const std::string text = "chr1\t5\t9\tchr2\t1\t2\t\t0.0\t+\t-\t77\nchr1\t5\t9\tchr2\t1\t2\tS\t0.0\t+\t-\t77\nchr1\t4.5\t9\nchr1";  // (no last newline)
    size_t pool_bytes = 0, count = 0;
    int plain = 1;
    CHECK(sdf_line_records((const uint8_t *)text.data(), text.size(), nullptr, 0, &pool_bytes, nullptr, 0, &count, nullptr) == SDF_OK);
    CHECK(count == 4 && pool_bytes % 16 == 0 && pool_bytes >= text.size() - 3 && pool_bytes <= text.size() + 60);
    std::vector<uint8_t> pool(pool_bytes);
    std::vector<sdf_line_rec> recs(count);
    CHECK(sdf_line_records((const uint8_t *)text.data(), text.size(), pool.data(), pool_bytes - 1, &pool_bytes, recs.data(), count, &count, &plain) == SDF_ERR_INVALID);
    CHECK(sdf_line_records((const uint8_t *)text.data(), text.size(), pool.data(), pool_bytes, &pool_bytes, recs.data(), count - 1, &count, &plain) == SDF_ERR_INVALID);
    CHECK(sdf_line_records((const uint8_t *)text.data(), text.size(), pool.data(), pool_bytes, &pool_bytes, recs.data(), count, &count, &plain) == SDF_OK);
    CHECK(plain == 0);
    // fields 9 / 10 of line 0 are "\t-" and "\t77", of line 1 "\t+" and "\t-": reversed ranks, so "\t-" (0x2d) is in front of "\t+" (0x2b)
    CHECK(recs[0].key[1] < recs[1].key[1] && recs[2].key[1] > recs[1].key[1]);  // (a missing field is empty: the last of the reversed)
    CHECK(recs[0].key[0] == recs[1].key[0] && recs[0].key[3] == recs[1].key[3] && recs[2].key[3] < recs[0].key[3]);
    CHECK(recs[2].key[4] < recs[0].key[4] && recs[3].key[4] < recs[2].key[4]);  // (ranks: 0 < 4.5 < 5)
    std::vector<uint32_t> order(4), flags(4);
    size_t kept = 0;
    sdf_line_rec bad = recs[3];
    bad.off += 8;
    std::vector<sdf_line_rec> with_bad{recs[0], recs[1], bad};
    CHECK(sdf_line_order_host(pool.data(), pool_bytes, with_bad.data(), 3, order.data(), flags.data(), &kept) == SDF_ERR_INVALID);
    with_bad[2] = recs[3], with_bad[2].len = (uint32_t)(pool_bytes - recs[3].off + 1);
    CHECK(sdf_line_order_host(pool.data(), pool_bytes, with_bad.data(), 3, order.data(), flags.data(), &kept) == SDF_ERR_INVALID);
    with_bad[2] = recs[3], with_bad[2].reserved = 1;
    CHECK(sdf_line_order_host(pool.data(), pool_bytes, with_bad.data(), 3, order.data(), flags.data(), &kept) == SDF_ERR_INVALID);
    CHECK(sdf_line_order_host(nullptr, 0, nullptr, 0, nullptr, nullptr, &kept) == SDF_OK && kept == 0);
    CHECK(sdf_line_order_host(nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr) == SDF_ERR_INVALID);
  }
  printf("line order ok\n");
  return 0;
}
