// sdf_pair_recall_host (sedef_amd/csrc/sdf_recall_api.hip) in a program of its own, against the definition written out here --
// every gold record against every found record, a painted array per side -- on the edges of the rule and on random clustered
// records: built with -fsanitize=address,undefined on the host side and run by tests/test_pair_recall_cpu.py, on the CPU.  Exit
// status 0 and "pair recall ok" when every statement holds; a finding makes the sanitizer's runtime end the program itself.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../include/sedef_hip.h"

#define CHECK(cond)                                               \
  do {                                                            \
    if (!(cond)) {                                                \
      fprintf(stderr, "line %d: %s fails\n", __LINE__, #cond);    \
      return 1;                                                   \
    }                                                             \
  } while (0)

namespace {
struct End {
  int chr, start, end;
  unsigned strand;
};
End end_of(const sdf_pair_rec &r, int e) { return e ? End{r.chr2, r.start2, r.end2, (r.flags >> 1) & 1u} : End{r.chr1, r.start1, r.end1, r.flags & 1u}; }
bool meets(const End &a, const End &b, bool ignore) {
  return a.chr == b.chr && std::min(a.end, b.end) - std::max(a.start, b.start) >= 1 && (ignore || a.strand == b.strand);
}
void paint(std::vector<char> &p, const End &g, const End &f) {
  for (int x = std::max(g.start, f.start); x < std::min(g.end, f.end); x++) p[(size_t)(x - g.start)] = 1;
}
sdf_pair_recall_rec definition(const sdf_pair_rec &g, const std::vector<sdf_pair_rec> &found, bool ignore) {
  const End g1 = end_of(g, 0), g2 = end_of(g, 1);
  std::vector<char> p1((size_t)(g1.end - g1.start), 0), p2((size_t)(g2.end - g2.start), 0);
  sdf_pair_recall_rec R{0u, 0, 0, 0u};
  size_t listed = 0;
  for (const sdf_pair_rec &f : found) {
    const End f1 = end_of(f, 0), f2 = end_of(f, 1);
    const bool direct = meets(g1, f1, ignore) && meets(g2, f2, ignore), cross = meets(g1, f2, ignore) && meets(g2, f1, ignore);
    if (direct) paint(p1, g1, f1), paint(p2, g2, f2);
    if (cross) paint(p1, g1, f2), paint(p2, g2, f1);
    R.n_hits += direct || cross;
    listed += (size_t)direct + (size_t)cross;
  }
  for (char c : p1) R.cov1 += c;
  for (char c : p2) R.cov2 += c;
  if (listed > SDF_RECALL_CAP) R.flags = SDF_RECALL_WIDE;
  return R;
}
bool same(const sdf_pair_recall_rec &a, const sdf_pair_recall_rec &b) {
  return a.n_hits == b.n_hits && a.cov1 == b.cov1 && a.cov2 == b.cov2 && a.flags == b.flags;
}
}  // namespace

int main() {
  std::mt19937 rng(7);
  const auto upto = [&](int n) { return (int)(rng() % (unsigned)n); };
  for (int draw = 0; draw < 60; draw++) {
    const int ng = 1 + upto(60), nf = draw == 0 ? 0 : draw == 1 ? 2 * SDF_RECALL_CAP + 50 : upto(800);
    const int places[4][2][2] = {{{upto(3), upto(50000)}, {upto(3), upto(50000)}}, {{upto(3), upto(50000)}, {upto(3), upto(50000)}},
                                 {{upto(3), upto(50000)}, {upto(3), upto(50000)}}, {{upto(3), upto(50000)}, {upto(3), upto(50000)}}};
    const auto rec = [&](int longest) {
      const int f = draw == 1 ? 0 : upto(4), swap = upto(3) == 0;
      const int a1 = places[f][swap][1] + upto(2000), a2 = places[f][!swap][1] + upto(2000);
      return sdf_pair_rec{places[f][swap][0], a1, a1 + upto(longest), places[f][!swap][0], a2, a2 + upto(longest), upto(4) ? 0u : (unsigned)upto(4), 0u};
    };
    std::vector<sdf_pair_rec> gold, found;
    for (int i = 0; i < ng; i++) gold.push_back(rec(3000));
    for (int i = 0; i < nf; i++) found.push_back(rec(draw % 3 ? 2500 : 40));
    const uint32_t flags = draw & 1 ? 0u : SDF_RECALL_IGNORE_STRAND;
    std::vector<sdf_pair_recall_rec> out((size_t)ng);
    CHECK(sdf_pair_recall_host(gold.data(), gold.size(), found.data(), found.size(), flags, out.data()) == SDF_OK);
    bool wide = false;
    for (int g = 0; g < ng; g++) {
      CHECK(same(out[(size_t)g], definition(gold[(size_t)g], found, flags != 0)));
      wide |= (out[(size_t)g].flags & SDF_RECALL_WIDE) != 0;
    }
    if (draw == 1) CHECK(wide);  // (the lists beyond the cap were walked too)
  }
  // the refusals read nothing they should not: exact-size arrays, the bad record last
  std::vector<sdf_pair_rec> one{{0, 5, 9, 1, 5, 9, 0u, 0u}}, bad{{0, 5, 9, 1, 5, 9, 0u, 0u}, {0, 9, 5, 1, 5, 9, 0u, 0u}};
  std::vector<sdf_pair_recall_rec> out(2);
  CHECK(sdf_pair_recall_host(bad.data(), 2, one.data(), 1, 0, out.data()) == SDF_ERR_INVALID);
  CHECK(sdf_pair_recall_host(one.data(), 1, bad.data(), 2, 0, out.data()) == SDF_ERR_INVALID);
  CHECK(sdf_pair_recall_host(one.data(), 1, one.data(), 1, 8u, out.data()) == SDF_ERR_UNSUPPORTED);
  CHECK(sdf_pair_recall_host(nullptr, 0, nullptr, 0, 0, nullptr) == SDF_OK);
  printf("pair recall ok\n");
  return 0;
}
