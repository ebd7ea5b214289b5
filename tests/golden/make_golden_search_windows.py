#!/usr/bin/env python3
"""Generates tests/golden/search_windows_kat.json.gz: query / reference sequences and what the front half of the REFERENCE's
search() (src/search.cc:399-459) answers for every query minimizer with an empty tree.  The small driver below is ours; it
includes the reference's hash.h and sliding.h and is compiled here, into a temporary directory, against the reference's
unmodified src/hash.cc, src/sliding.cc, src/globals.cc and extern/format.cc where they lie.  The driver builds the two Index
objects, sets the reference index's threshold to the case's, answers relaxed_jaccard_estimate (src/util.cc:85, which needs
Boost.Math) from the case's table, takes query_size and limit from the reference's SlidingMap::add_to_query, looks the groups
up in the reference's Index, and states the seven steps of include/sedef_hip.h in its own words around them, without a tree.
Needs /root/reference (build container only); the fixture is data.

A case is {name, q, r, r_rc, same (query and reference are one sequence: r is not stored), k, w, sl, init_len, same_genome,
uppercase_seeds, threshold, limit, nq, windows}; a window is [query_size, flags, [candidates], [[start, end] ...]] (flags:
1 SHORT -- search() returned before anything --, 2 NOLIMIT -- query_size is beyond the table, the driver stops there)."""
import gzip
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = os.environ.get("SEDEF_REFERENCE", "/root/reference")

DRIVER = r"""
#include <algorithm>
#include <array>
#include <cstdio>
#include <iostream>
#include <memory>
#include <string>
#include <vector>
#include "common.h"
#include "hash.h"
#include "sliding.h"
using namespace std;
// src/util.cc does not build without Boost: the two functions of it that the reference's classes call
string rc(const string &s) {
  string r(s.size(), 'N');
  for (size_t i = 0; i < s.size(); i++) r[i] = rev_dna(s[s.size() - 1 - i]);
  return r;
}
static vector<int> g_table;  // the case's limit by query_size
int relaxed_jaccard_estimate(int s, int kmer_size, unordered_map<int, int> &mm) { return s >= 0 && s < (int)g_table.size() ? g_table[s] : 1; }

struct Case {
  int k, w, sl, r_rc, init_len, same_genome, uppercase_seeds, same;
  unsigned threshold;
};

// steps 2 to 4 of include/sedef_hip.h for window i: the members go into `win` (the reference's SlidingMap counts query_size and
// looks the limit up), the positions of the seeding members' groups come back ascending and distinct
static vector<int> window_positions(const Case &c, const Index &query, const Index &ref, size_t i, SlidingMap &win) {
  const vector<Minimizer> &m = query.minimizers;
  const long long floor = (long long)m[i].loc + c.init_len;
  vector<int> pos;
  for (size_t j = i; j < m.size() && m[j].loc <= floor; j++) {
    win.add_to_query(m[j].hash);
    if (c.uppercase_seeds && m[j].hash.status != Hash::Status::HAS_UPPERCASE) continue;
    const auto group = ref.index.find(m[j].hash);
    if (group == ref.index.end() || group->second.size() >= ref.threshold) continue;
    for (int p : group->second)
      if (!c.same_genome || p >= floor) pos.push_back(p);
  }
  sort(pos.begin(), pos.end());
  pos.erase(unique(pos.begin(), pos.end()), pos.end());
  return pos;
}

// steps 6 and 7: the spans of L positions that lie within init_len, overlapping ones joined, cut at `floor` for one genome
static vector<array<int, 2>> window_intervals(const Case &c, const vector<int> &pos, int L, long long floor) {
  vector<array<int, 2>> spans;
  const int n = (int)pos.size();
  for (int a = 0; a + L <= n; a++) {
    const int lo_pos = pos[a], hi_pos = pos[a + L - 1];
    if (hi_pos - lo_pos > c.init_len) continue;
    const int x = hi_pos - c.init_len + 1 > 0 ? hi_pos - c.init_len + 1 : 0, y = lo_pos + 1;
    if (spans.empty() || x >= spans.back()[1]) spans.push_back({x, y});
    else if (y > spans.back()[1]) spans.back()[1] = y;
  }
  if (!c.same_genome) return spans;
  vector<array<int, 2>> cut;
  for (auto s : spans) {
    if (s[0] < floor) s[0] = (int)floor;
    if (s[0] <= s[1]) cut.push_back(s);
  }
  return cut;
}

int main() {
  Case c;
  size_t n_limit;
  while (cin >> c.k >> c.w >> c.sl >> c.r_rc >> c.init_len >> c.same_genome >> c.uppercase_seeds >> c.same >> c.threshold >> n_limit) {
    g_table.assign(n_limit, 0);
    for (auto &x : g_table) cin >> x;
    string qs, rs;
    cin >> qs;
    if (!c.same) cin >> rs;
    auto query = make_shared<Index>(make_shared<Sequence>("q", qs, false), c.k, c.w, c.sl != 0);
    auto ref = c.same ? query : make_shared<Index>(make_shared<Sequence>("r", rs, c.r_rc != 0), c.k, c.w, c.sl != 0);
    ref->threshold = c.threshold;
    printf("C %zu\n", query->minimizers.size());
    for (size_t i = 0; i < query->minimizers.size(); i++) {
      const long long floor = (long long)query->minimizers[i].loc + c.init_len;
      if (floor > (long long)qs.size()) {  // step 1
        printf("0 1 0 0\n");
        continue;
      }
      SlidingMap win(c.k);
      const vector<int> pos = window_positions(c, *query, *ref, i, win);
      const bool nolimit = win.query_size >= (int)n_limit;  // step 5
      vector<array<int, 2>> spans;
      if (!nolimit) spans = window_intervals(c, pos, (int)win.limit, floor);
      printf("%d %d %zu %zu", win.query_size, nolimit ? 2 : 0, pos.size(), spans.size());
      for (int p : pos) printf(" %d", p);
      for (auto &s : spans) printf(" %d %d", s[0], s[1]);
      printf("\n");
    }
  }
  return 0;
}
"""


def build_driver(tmp):
    src = os.path.join(tmp, "search_driver.cc")
    exe = os.path.join(tmp, "search_driver")
    with open(src, "w") as f:
        f.write(DRIVER)
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-w", "-I" + REF, "-I" + os.path.join(REF, "src"), "-o", exe, src,
                           os.path.join(REF, "src", "hash.cc"), os.path.join(REF, "src", "sliding.cc"),
                           os.path.join(REF, "src", "globals.cc"), os.path.join(REF, "extern", "format.cc")])
    return exe


def run_driver(exe, cases):
    lines = []
    for c in cases:
        head = [c["k"], c["w"], c["sl"], c["r_rc"], c["init_len"], c["same_genome"], c["uppercase_seeds"], c["same"], c["threshold"],
                len(c["limit"])] + c["limit"]
        lines.append(" ".join(str(x) for x in head))
        lines.append(c["q"])
        if not c["same"]:
            lines.append(c["r"])
    tok = iter(subprocess.run([exe], input=("\n".join(lines) + "\n").encode(), stdout=subprocess.PIPE, check=True).stdout.split())
    out = []
    for _ in cases:
        assert next(tok) == b"C"
        windows = []
        for _ in range(int(next(tok))):
            qsz, flags, nc, nt = int(next(tok)), int(next(tok)), int(next(tok)), int(next(tok))
            cand = [int(next(tok)) for _ in range(nc)]
            windows.append([qsz, flags, cand, [[int(next(tok)), int(next(tok))] for _ in range(nt)]])
        out.append(windows)
    assert next(tok, None) is None
    return out


LETTERS = np.frombuffer(b"ACGT", np.uint8)


def mutate(rng, a, rate):
    """Substitutions at `rate`, and a few single-base deletions and insertions."""
    a = a.copy()
    hit = rng.random(len(a)) < rate
    a[hit] = (a[hit] + rng.integers(1, 4, int(hit.sum()))) % 4
    for _ in range(int(rng.integers(0, 3))):
        at = int(rng.integers(1, len(a) - 1))
        a = np.delete(a, at) if rng.random() < 0.5 else np.insert(a, at, int(rng.integers(0, 4)))
    return a


def compose(rng, total, units, copies, rate):
    """A random sequence of about `total` bases with `copies` mutated copies of the units spliced in."""
    parts, left = [], total
    for _ in range(copies):
        gap = int(rng.integers(20, max(21, total // (2 * copies))))
        parts += [rng.integers(0, 4, gap), mutate(rng, units[int(rng.integers(0, len(units)))], rate)]
    parts.append(rng.integers(0, 4, int(rng.integers(30, 120))))
    return np.concatenate(parts)


def text(rng, a, lower=0, n_runs=0):
    """Codes as FASTA characters: `lower` soft-masked stretches and `n_runs` runs of N, each longer than a window."""
    s = LETTERS[a].copy()
    for _ in range(lower):
        at, ln = int(rng.integers(0, len(s) - 80)), int(rng.integers(40, 160))
        s[at:at + ln] |= 0x20
    for _ in range(n_runs):
        at, ln = int(rng.integers(0, len(s) - 60)), int(rng.integers(30, 60))
        s[at:at + ln] = ord("N") if rng.random() < 0.7 else ord("n")
    return s.tobytes().decode()


def table(n, frac, floor=1):
    return [max(floor, int(s * frac)) for s in range(n)]


def make_cases(rng):
    cases = []

    def add(name, q, r, **kw):
        c = dict(name=name, q=q, r=r, r_rc=0, same=0, k=12, w=16, sl=1, init_len=300, same_genome=0, uppercase_seeds=1,
                 threshold=1 << 31, limit=table(120, 0.12))
        c.update(kw)
        if c["same"]:
            c["r"] = ""
        cases.append(c)

    # query and reference share mutated repeats; soft-masked stretches and runs of N on both sides
    for it in range(22):
        units = [rng.integers(0, 4, int(rng.integers(250, 700))) for _ in range(3)]
        rate = float(rng.choice([0.01, 0.03, 0.06]))
        q = text(rng, compose(rng, 2600, units, 4, rate), lower=5, n_runs=2)
        r = text(rng, compose(rng, 3200, units, 6, rate), lower=6, n_runs=2)
        init_len = int(rng.choice([150, 300, 500]))
        frac = float(rng.choice([0.05, 0.1, 0.2]))
        add("repeats %d" % it, q, r, init_len=init_len, limit=table(160, frac), uppercase_seeds=int(it % 3 != 0),
            sl=int(it % 5 != 4), w=int(rng.choice([8, 16])), threshold=int(rng.choice([1 << 31, 1 << 31, 4, 3])))
    # a reversed reference: the reverse complement of the reference shares the repeats
    units = [rng.integers(0, 4, 500) for _ in range(2)]
    q = text(rng, compose(rng, 2400, units, 4, 0.03), lower=3, n_runs=1)
    r = text(rng, (3 - compose(rng, 3000, units, 5, 0.03))[::-1], lower=3, n_runs=1)
    add("reversed reference", q, r, r_rc=1, limit=table(120, 0.1))
    # the sequence against itself: candidates only from qs + init_len on
    for it in range(4):
        units = [rng.integers(0, 4, int(rng.integers(300, 600))) for _ in range(2)]
        s = text(rng, compose(rng, 4000, units, 7, 0.03), lower=4, n_runs=1)
        add("same genome %d" % it, s, "", same=1, same_genome=1, init_len=int(rng.choice([200, 400])), limit=table(140, 0.08),
            uppercase_seeds=int(it != 3))
    # L = 1 everywhere: every candidate passes; a table too short for most windows; tandem repeats (one key many times a window)
    units = [rng.integers(0, 4, 400) for _ in range(2)]
    q, r = text(rng, compose(rng, 1500, units, 3, 0.02)), text(rng, compose(rng, 1800, units, 3, 0.02))
    add("limit 1", q, r, limit=[1] * 100, init_len=200)
    add("short table", q, r, limit=table(14, 0.2), init_len=200)
    unit = rng.integers(0, 4, 37)
    tandem = np.tile(unit, 40)
    q = text(rng, np.concatenate([rng.integers(0, 4, 200), mutate(rng, tandem, 0.01), rng.integers(0, 4, 300)]), lower=2)
    r = text(rng, np.concatenate([rng.integers(0, 4, 300), mutate(rng, tandem, 0.02), rng.integers(0, 4, 200)]), lower=2)
    add("tandem repeats", q, r, limit=table(100, 0.15), init_len=250)
    add("tandem repeats, threshold 20", q, r, limit=table(100, 0.15), init_len=250, threshold=20, uppercase_seeds=0)
    # sequences shorter than init_len, and without a minimizer
    add("shorter than init_len", text(rng, rng.integers(0, 4, 120)), text(rng, rng.integers(0, 4, 200)), init_len=300)
    add("no minimizer", "ACGTACGTACGTACG", text(rng, rng.integers(0, 4, 200)))
    return cases


def main():
    rng = np.random.default_rng(20261019)
    cases = make_cases(rng)
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(tmp)
        for c, windows in zip(cases, run_driver(exe, cases)):
            c.update(nq=len(windows), windows=windows)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import minim_model as M
    n_windows = n_with = n_two = n_dup = n_status = 0
    flags = set()
    for c in cases:
        mins = M.get_minimizers(c["q"].encode(), c["k"], c["w"], bool(c["sl"]))
        assert len(mins) == c["nq"], c["name"]
        n_status += {1, 2} <= {m[2] for m in mins}
        locs = [m[1] for m in mins]
        for i, (qsz, fl, cand, T) in enumerate(c["windows"]):
            n_windows += 1
            n_with += len(T) > 0
            n_two += len(T) >= 2
            flags.add(fl)
            if fl != 1:
                members = [(m[2], m[0]) for m, loc in zip(mins[i:], locs[i:]) if loc - locs[i] <= c["init_len"]]
                assert len(set(members)) == qsz, (c["name"], i)
                n_dup += len(set(members)) < len(members)
    print("windows %d, with an interval %d, with two and more %d, with duplicate keys %d; cases with status 1 and 2: %d; flags %s"
          % (n_windows, n_with, n_two, n_dup, n_status, sorted(flags)))
    assert 3 * n_with >= n_windows and n_two >= 50 and n_dup >= 20 and n_status >= 20 and flags == {0, 1, 2}
    path = os.path.join(ROOT, "tests", "golden", "search_windows_kat.json.gz")
    blob = json.dumps(dict(source="reference search() front half (src/search.cc:399-459, empty tree) via the driver of "
                                  "tests/golden/make_golden_search_windows.py", cases=cases), separators=(",", ":")).encode()
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(blob)
    size = os.path.getsize(path)
    print("wrote %s: %d cases, %d bytes (%d uncompressed)" % (path, len(cases), size, len(blob)))
    assert size <= 945356, size  # (no larger than the largest fixture of tests/golden)


if __name__ == "__main__":
    sys.exit(main())
