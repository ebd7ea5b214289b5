#!/usr/bin/env python3
"""Generates tests/golden/search_roll_kat.json.gz: query / reference sequences, the reference intervals of every query window
and what the first loop of the REFERENCE's search_in_reference_interval (src/search.cc:274-314, "Roll until we find best
inital match") answers for each of them.  src/search.cc does not build here (Boost), so the small driver below states that
walk in our own words around the reference's own SlidingMap (add_to_query, add_to_reference, remove_from_reference, jaccard)
and Index::find_minimizers; the intervals come from the front-half driver of make_golden_search_windows.py, whose functions
this driver takes over as they are.  It is compiled here, into a temporary directory, against the reference's unmodified
src/hash.cc, src/sliding.cc, src/globals.cc and extern/format.cc where they lie.  Needs /root/reference (build container
only); the fixture is data.

SlidingMap::remove dereferences storage.lower_bound(h) without asking whether it is end(): before every
remove_from_reference the driver looks into the public `storage`, and where the reference would read end() it skips the call
and counts it (include/sedef_hip.h: such a remove is a no-op).

A case is {name, q, r, r_rc, same, k, w, sl, init_len, same_genome, uppercase_seeds, threshold, limit, nq, windows, counters};
a window is [query_size, flags, [[start, end, ref_start, ref_end, winnow_start, winnow_end, jaccard] ...]].  counters, per
case: dup_removes (removes that were no-ops because a duplicate had cleared the bit), adds_on_boundary (adds that hit B
exactly), negative (intervals in which I went below 0), status2 (reference records of status 2 inside a span), clamped
(intervals whose first e was clamped at len_r), ended_at_len_r (intervals the walk left because e reached len_r)."""
import gzip
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
import make_golden_search_windows as W  # noqa: E402

COUNTERS = ("dup_removes", "adds_on_boundary", "negative", "status2", "clamped", "ended_at_len_r")

# the front-half driver up to its main(): Case, window_positions, window_intervals
DRIVER = W.DRIVER[:W.DRIVER.index("int main()")] + r"""
static long long n_dup, n_onb, n_neg, n_st2, n_clamp, n_atend;

// the walk of include/sedef_hip.h for one interval, on a copy of the window's map
static void roll(const Index &ref, SlidingMap winnow, int init_len, int t_start, int t_end) {
  const vector<Minimizer> &m = ref.minimizers;
  const int len_r = (int)ref.seq->seq.size(), nr = (int)m.size();
  bool negative = false;
  auto add = [&](const Hash &h) {
    if (h.status == Hash::Status::HAS_N) n_st2++;
    else if (winnow.boundary != winnow.storage.end() && winnow.boundary->first == h && !(winnow.boundary->second & 2)) n_onb++;
    winnow.add_to_reference(h);
  };
  auto remove = [&](const Hash &h) {
    if (h.status != Hash::Status::HAS_N) {
      auto it = winnow.storage.lower_bound(h);
      const bool absent = it == winnow.storage.end();
      if (absent || !(it->first == h) || !(it->second & 2)) n_dup++;
      if (absent) return;  // (the reference would read end() here)
    }
    winnow.remove_from_reference(h);
  };
  auto score = [&]() {
    negative |= winnow.intersection < 0;
    return winnow.jaccard();
  };
  int s = t_start, e = min(t_start + init_len, len_r);
  if (t_start + init_len > len_r) n_clamp++;
  int ws = ref.find_minimizers(s), we = ws;
  while (we < nr && m[we].loc < e) add(m[we++].hash);
  int best[5] = {s, e, ws, we, score()};
  while (s < t_end && e < len_r) {
    if (ws < nr && m[ws].loc <= s) remove(m[ws++].hash);
    if (we < nr && m[we].loc == e) add(m[we++].hash);
    const int now = score();
    if (now > best[4]) best[0] = s, best[1] = e, best[2] = ws, best[3] = we, best[4] = now;
    s++, e++;
  }
  if (s < t_end && e == len_r && t_start + init_len < len_r) n_atend++;
  n_neg += negative;
  printf(" %d %d %d %d %d", best[0], best[1], best[2], best[3], best[4]);
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
    n_dup = n_onb = n_neg = n_st2 = n_clamp = n_atend = 0;
    printf("C %zu\n", query->minimizers.size());
    for (size_t i = 0; i < query->minimizers.size(); i++) {
      const long long floor = (long long)query->minimizers[i].loc + c.init_len;
      if (floor > (long long)qs.size()) {
        printf("0 1 0\n");
        continue;
      }
      SlidingMap win(c.k);
      const vector<int> pos = window_positions(c, *query, *ref, i, win);
      const bool nolimit = win.query_size >= (int)n_limit;
      vector<array<int, 2>> spans;
      if (!nolimit) spans = window_intervals(c, pos, (int)win.limit, floor);
      printf("%d %d %zu", win.query_size, nolimit ? 2 : 0, spans.size());
      for (auto &sp : spans) {
        printf(" %d %d", sp[0], sp[1]);
        roll(*ref, win, c.init_len, sp[0], sp[1]);
      }
      printf("\n");
    }
    printf("K %lld %lld %lld %lld %lld %lld\n", n_dup, n_onb, n_neg, n_st2, n_clamp, n_atend);
  }
  return 0;
}
"""


def build_driver(tmp):
    src = os.path.join(tmp, "roll_driver.cc")
    exe = os.path.join(tmp, "roll_driver")
    with open(src, "w") as f:
        f.write(DRIVER)
    ref = W.REF
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-w", "-I" + ref, "-I" + os.path.join(ref, "src"), "-o", exe, src,
                           os.path.join(ref, "src", "hash.cc"), os.path.join(ref, "src", "sliding.cc"),
                           os.path.join(ref, "src", "globals.cc"), os.path.join(ref, "extern", "format.cc")])
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
            qsz, flags, nt = int(next(tok)), int(next(tok)), int(next(tok))
            windows.append([qsz, flags, [[int(next(tok)) for _ in range(7)] for _ in range(nt)]])
        assert next(tok) == b"K"
        out.append((windows, {name: int(next(tok)) for name in COUNTERS}))
    assert next(tok, None) is None
    return out


def short_repeats(rng, total, unit_len, copies, rate):
    """About `total` bases in which a few short units come again and again, lightly mutated."""
    units = [rng.integers(0, 4, unit_len) for _ in range(2)]
    parts = []
    for _ in range(copies):
        parts += [rng.integers(0, 4, int(rng.integers(3, max(4, total // copies - unit_len)))), W.mutate(rng, units[int(rng.integers(0, 2))], rate)]
    return np.concatenate(parts), units


def make_cases(rng):
    cases = []

    def add(name, q, r, **kw):
        c = dict(name=name, q=q, r=r, r_rc=0, same=0, k=12, w=16, sl=1, init_len=700, same_genome=0, uppercase_seeds=1,
                 threshold=1 << 31, limit=W.table(200, 0.1))
        c.update(kw)
        if c["same"]:
            c["r"] = ""
        cases.append(c)

    # small k, small w, short repeats: keys come again inside one window (duplicate removes, adds onto the boundary, I < 0)
    for it in range(40):
        k, w = int(rng.integers(3, 6)), int(rng.integers(2, 5))
        init_len = int(rng.choice([12, 20, 30, 45]))
        total = int(rng.integers(150, 420))
        qa, units = short_repeats(rng, total, int(rng.integers(8, 30)), int(rng.integers(4, 9)), 0.04)
        ra = np.concatenate([W.mutate(rng, units[int(rng.integers(0, 2))], 0.05) if rng.random() < 0.6 else rng.integers(0, 4, 9)
                             for _ in range(int(rng.integers(6, 16)))])
        q = W.text(rng, qa, lower=int(it % 3 == 0) * 2)
        r = W.text(rng, ra, lower=int(it % 4 == 0), n_runs=int(it % 5 == 1) if len(ra) > 80 else 0)
        same = it % 8 == 7
        add("small %d" % it, q, r, k=k, w=w, init_len=init_len, same=int(same), same_genome=int(same), sl=int(it % 6 != 5),
            uppercase_seeds=int(it % 2), limit=W.table(80, float(rng.choice([0.1, 0.25, 0.4]))))
    # a reference shorter than init_len (every first e is clamped) and one that ends inside most intervals
    for it in range(4):
        qa, units = short_repeats(rng, 260, 14, 6, 0.03)
        ra = np.concatenate([units[0], rng.integers(0, 4, 5), units[1], units[0]][:2 + it])
        add("short reference %d" % it, W.text(rng, qa), W.text(rng, ra), k=4, w=3, init_len=[60, 40, 25, 20][it], uppercase_seeds=0,
            limit=W.table(80, 0.2))
    # the program's own sizes: k 12, w 16, init_len 700; one genome; a reversed reference
    for it in range(2):
        units = [rng.integers(0, 4, int(rng.integers(800, 1100))) for _ in range(2)]
        q = W.text(rng, W.compose(rng, 3200, units, 3, 0.03), lower=3, n_runs=1)
        r = W.text(rng, W.compose(rng, 3600, units, 4, 0.03), lower=3, n_runs=1)
        add("k12 %d" % it, q, r, limit=W.table(200, [0.08, 0.15][it]), uppercase_seeds=int(it == 0))
    units = [rng.integers(0, 4, 900) for _ in range(2)]
    q = W.text(rng, W.compose(rng, 3000, units, 3, 0.03), lower=2, n_runs=1)
    r = W.text(rng, (3 - W.compose(rng, 3400, units, 4, 0.03))[::-1], lower=2, n_runs=1)
    add("k12 reversed reference", q, r, r_rc=1)
    for it in range(2):
        units = [rng.integers(0, 4, 850) for _ in range(2)]
        s = W.text(rng, W.compose(rng, 5200, units, 5, 0.02), lower=3, n_runs=1)
        add("k12 same genome %d" % it, s, "", same=1, same_genome=1, uppercase_seeds=int(it == 0), limit=W.table(200, 0.1))
    return cases


def main():
    rng = np.random.default_rng(20261020)
    cases = make_cases(rng)
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(tmp)
        for c, (windows, counters) in zip(cases, run_driver(exe, cases)):
            c.update(nq=len(windows), windows=windows, counters=counters)
    total = {name: sum(c["counters"][name] for c in cases) for name in COUNTERS}
    n_int = sum(len(w[2]) for c in cases for w in c["windows"])
    n_moved = sum(t[2] != t[0] for c in cases for w in c["windows"] for t in w[2])
    k12 = [c for c in cases if c["k"] == 12]
    print("intervals %d (k = 12: %d), best not at the start %d; counters %s"
          % (n_int, sum(len(w[2]) for c in k12 for w in c["windows"]), n_moved, total))
    assert all(v > 0 for v in total.values()), total
    assert n_int >= 2000 and 5 * n_moved >= n_int
    assert all(sum(len(w[2]) for w in c["windows"]) > 20 for c in k12) and any(c["same_genome"] for c in k12) and any(c["r_rc"] for c in k12)
    path = os.path.join(ROOT, "tests", "golden", "search_roll_kat.json.gz")
    blob = json.dumps(dict(source="reference SlidingMap and Index::find_minimizers, the roll of src/search.cc:274-314 via the driver "
                                  "of tests/golden/make_golden_search_roll.py", cases=cases), separators=(",", ":")).encode()
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(blob)
    size = os.path.getsize(path)
    print("wrote %s: %d cases, %d bytes (%d uncompressed)" % (path, len(cases), size, len(blob)))
    assert size <= 300000, size


if __name__ == "__main__":
    sys.exit(main())
