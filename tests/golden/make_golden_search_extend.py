#!/usr/bin/env python3
"""Generates tests/golden/search_extend_kat.json.gz: the cases of make_golden_search_roll.py (and some of one genome against
itself whose overlap test fires), every interval rolled as there and then grown to its hit by the REFERENCE's extend()
(src/search.cc:95-259).  src/search.cc does not build here (Boost), so the small driver below states the roll and the
extension in our own words around the reference's own SlidingMap (add_to_query, remove_from_query, add_to_reference,
remove_from_reference, jaccard, its copy constructor for best_winnow) and Index; the front half is the driver of
make_golden_search_windows.py, taken over as it is.  It is compiled here, into a temporary directory, with -DNDEBUG (the
SlidingMap as it behaves, not as it asserts) against the reference's unmodified src/hash.cc, src/sliding.cc, src/globals.cc
and extern/format.cc where they lie.  Needs /root/reference (build container only); the fixture is data.

The guard.  SlidingMap reads past its map in four places: remove() dereferences lower_bound(h) == end(); add() and remove()
dereference a boundary that is end() while query_size > 0; add_to_query() steps the boundary past the last stored key; and
remove() may step it there, after which the next call reads it.  include/sedef_hip.h defines each of them (a no-op at that
point); the reference does not, so before every call the driver looks into the public `storage` and `boundary`, and where the
reference would get there it ends the interval and marks the case.  Such a case is DISCARDED and drawn again: every committed
hit is the reference's own answer.  (In the roll in front -- where only the first can happen -- the call is skipped, as in
make_golden_search_roll.py, which counts those; this driver does not count them again.)  The guard is a mark per case, not a
count: main() prints how many cases were drawn again.

A case is the roll fixture's with max_error, max_edit_error, max_sd_size and counters; a window is [query_size, flags,
[[start, end, ref_start, ref_end, winnow_start, winnow_end, jaccard, hit ...] ...]] with hit = [flags, query_start, query_end,
ref_start, ref_end, jaccard, q_winnow_start, q_winnow_end, r_winnow_start, r_winnow_end]; flags 1: not extended (the roll's
jaccard is below 0), 4: a step needed limit[s] beyond the table (the rest is zero).  counters, per case: undos (extensions
taken back), false_add_undos (those of them in which an add_to_query had returned false: the undo then clears a bit its do
never set), stop_len / stop_ratio / stop_overlap (rounds ended by aln_len > max_match, by the length ratio, by the overlap of
one genome), at_end (hits with a winnow range at an end of its sequence)."""
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
import make_golden_search_roll as R  # noqa: E402
import make_golden_search_windows as W  # noqa: E402

COUNTERS = ("undos", "false_add_undos", "stop_len", "stop_ratio", "stop_overlap", "at_end")
SKIPPED, NOLIMIT = 1, 4

DRIVER = W.DRIVER[:W.DRIVER.index("int main()")] + r"""
static long long n_undo, n_false_undo, n_stop_len, n_stop_ratio, n_stop_overlap, n_at_end;
static bool guard, nolimit;
static double max_error, max_edit_error;
static int max_sd_size;

// the four calls, each behind a look at what it would read
struct Guarded {
  SlidingMap &m;
  bool lost() const { return m.query_size > 0 && m.boundary == m.storage.end(); }
  bool add_to_query(const Hash &h) {  // false: the reference's add() returned false
    auto it = m.storage.find(h);
    const bool fresh = it == m.storage.end();
    if (!fresh && (it->second & 1)) return m.add_to_query(h), false;
    if (lost()) return guard = true, true;
    if (m.boundary != m.storage.end() && !(fresh && h < m.boundary->first) && next(m.boundary) == m.storage.end() &&
        !(fresh && m.boundary->first < h))
      return guard = true, true;
    if (m.query_size + 1 >= (int)g_table.size()) return nolimit = true, true;
    m.add_to_query(h);
    return true;
  }
  void remove(const Hash &h, int bit) {
    auto it = m.storage.lower_bound(h);
    if (it == m.storage.end()) return void(guard = true);
    if (it->first == h && (it->second & bit)) {
      if (lost()) return void(guard = true);
      if (h <= m.boundary->first && it->second == bit && next(m.boundary) == m.storage.end()) return void(guard = true);
    }
    if (bit == 1) m.remove_from_query(h);
    else m.remove_from_reference(h);
  }
  void add_to_reference(const Hash &h) {
    if (h.status == Hash::Status::HAS_N) return;
    auto it = m.storage.find(h);
    if (!(it != m.storage.end() && (it->second & 2)) && lost()) return void(guard = true);
    m.add_to_reference(h);
  }
  void remove_from_query(const Hash &h) { remove(h, 1); }
  void remove_from_reference(const Hash &h) {
    if (h.status != Hash::Status::HAS_N) remove(h, 2);
  }
};

// src/search.cc:95-259 for one rolled interval: the do and undo steps in the reference's order
static void extend(const Index &query, const Index &ref, SlidingMap &best, int qws, int qwe, int rws, int rwe, bool same_genome) {
  const vector<Minimizer> &q = query.minimizers, &r = ref.minimizers;
  const int nq = (int)q.size(), nr = (int)r.size(), len_q = (int)query.seq->seq.size(), len_r = (int)ref.seq->seq.size();
  Guarded g{best};
  int qs, qe, rs, re;
  bool false_add = false;
  auto do_query_right = [&]() {
    false_add |= !g.add_to_query(q[qwe++].hash);
    qe = qwe < nq ? q[qwe].loc : len_q;
  };
  auto undo_query_right = [&]() {
    g.remove_from_query(q[--qwe].hash);
    qe = q[qwe].loc;
  };
  auto do_ref_right = [&]() {
    g.add_to_reference(r[rwe++].hash);
    re = rwe < nr ? r[rwe].loc : len_r;
  };
  auto undo_ref_right = [&]() {
    g.remove_from_reference(r[--rwe].hash);
    re = r[rwe].loc;
  };
  auto do_query_left = [&]() {
    false_add |= !g.add_to_query(q[--qws].hash);
    qs = qws ? q[qws - 1].loc + 1 : 0;
  };
  auto undo_query_left = [&]() {
    qs = q[qws].loc + 1;
    g.remove_from_query(q[qws++].hash);
  };
  auto do_ref_left = [&]() {
    g.add_to_reference(r[--rws].hash);
    rs = rws ? r[rws - 1].loc + 1 : 0;
  };
  auto undo_ref_left = [&]() {
    rs = r[rws].loc + 1;
    g.remove_from_reference(r[rws++].hash);
  };
  qs = qws ? q[qws - 1].loc + 1 : 0, qe = qwe < nq ? q[qwe].loc : len_q;
  rs = rws ? r[rws - 1].loc + 1 : 0, re = rwe < nr ? r[rwe].loc : len_r;
  const double MAX_GAP_ERROR = max_error - max_edit_error;
  while (!guard && !nolimit) {
    int max_match = min(max_sd_size, same_genome ? int((1.0 / MAX_GAP_ERROR + .5) * abs(qs - rs)) : max_sd_size);
    int aln_len = max(qe - qs, re - rs), seq_len = min(qe - qs, re - rs);
    if (aln_len > max_match) {
      n_stop_len++;
      break;
    }
    if (pct(seq_len, aln_len) < 100 * (1 - 2 * MAX_GAP_ERROR)) {
      n_stop_ratio++;
      break;
    }
    if (same_genome) {
      int overlap = qe - rs;
      if (overlap > 0 && pct(overlap, re - rs) > 100 * max_error) {
        n_stop_overlap++;
        break;
      }
    }
    bool extended = false;
    for (int way = 0; way < 3 && !extended && !guard && !nolimit; way++) {  // both_both, both_right, both_left
      const bool left = way != 1, right = way != 2;
      if (left && (!qws || !rws)) continue;
      if (right && (rwe >= nr || qwe >= nq)) continue;
      false_add = false;
      if (left) do_query_left(), do_ref_left();
      if (right) do_query_right(), do_ref_right();
      if (guard || nolimit) break;
      if (best.jaccard() >= 0) {
        extended = true;
      } else {
        n_undo++, n_false_undo += false_add;
        if (right) undo_ref_right(), undo_query_right();
        if (left) undo_ref_left(), undo_query_left();
      }
    }
    if (!extended) break;
  }
  if (guard) return;
  if (nolimit) {
    printf(" 4 0 0 0 0 0 0 0 0 0");
    return;
  }
  n_at_end += !qws || !rws || qwe == nq || rwe == nr;
  printf(" 0 %d %d %d %d %d %d %d %d %d", qs, qe, rs, re, best.jaccard(), qws, qwe, rws, rwe);
}

// the walk of include/sedef_hip.h for one interval, on a copy of the window's map; then the extension on best_winnow
static void roll_extend(const Case &c, const Index &query, const Index &ref, SlidingMap winnow, int qws, int qwe, int t_start, int t_end) {
  const vector<Minimizer> &m = ref.minimizers;
  const int len_r = (int)ref.seq->seq.size(), nr = (int)m.size(), init_len = c.init_len;
  auto remove = [&](const Hash &h) {
    if (h.status != Hash::Status::HAS_N && winnow.storage.lower_bound(h) == winnow.storage.end()) return;  // (the reference would read end() here)
    winnow.remove_from_reference(h);
  };
  int s = t_start, e = min(t_start + init_len, len_r);
  int ws = ref.find_minimizers(s), we = ws;
  while (we < nr && m[we].loc < e) winnow.add_to_reference(m[we++].hash);
  SlidingMap best_winnow(winnow);
  int best[4] = {s, e, ws, we};
  while (s < t_end && e < len_r) {
    if (ws < nr && m[ws].loc <= s) remove(m[ws++].hash);
    if (we < nr && m[we].loc == e) winnow.add_to_reference(m[we++].hash);
    if (winnow.jaccard() > best_winnow.jaccard()) best[0] = s, best[1] = e, best[2] = ws, best[3] = we, best_winnow = winnow;
    s++, e++;
  }
  printf(" %d %d %d %d %d", best[0], best[1], best[2], best[3], best_winnow.jaccard());
  if (best_winnow.jaccard() < 0) {
    printf(" 1 0 0 0 0 0 0 0 0 0");
    return;
  }
  nolimit = false;
  extend(query, ref, best_winnow, qws, qwe, best[2], best[3], c.same_genome != 0);
}

int main() {
  Case c;
  size_t n_limit;
  while (cin >> c.k >> c.w >> c.sl >> c.r_rc >> c.init_len >> c.same_genome >> c.uppercase_seeds >> c.same >> c.threshold >> max_error >>
         max_edit_error >> max_sd_size >> n_limit) {
    g_table.assign(n_limit, 0);
    for (auto &x : g_table) cin >> x;
    string qs, rs;
    cin >> qs;
    if (!c.same) cin >> rs;
    auto query = make_shared<Index>(make_shared<Sequence>("q", qs, false), c.k, c.w, c.sl != 0);
    auto ref = c.same ? query : make_shared<Index>(make_shared<Sequence>("r", rs, c.r_rc != 0), c.k, c.w, c.sl != 0);
    ref->threshold = c.threshold;
    n_undo = n_false_undo = n_stop_len = n_stop_ratio = n_stop_overlap = n_at_end = 0;
    guard = false;
    printf("C %zu\n", query->minimizers.size());
    for (size_t i = 0; i < query->minimizers.size(); i++) {
      const long long floor = (long long)query->minimizers[i].loc + c.init_len;
      if (floor > (long long)qs.size()) {
        printf("0 1 0\n");
        continue;
      }
      SlidingMap win(c.k);
      const vector<int> pos = window_positions(c, *query, *ref, i, win);
      size_t qwe = i;
      while (qwe < query->minimizers.size() && query->minimizers[qwe].loc <= floor) qwe++;
      const bool nolim = win.query_size >= (int)n_limit;
      vector<array<int, 2>> spans;
      if (!nolim) spans = window_intervals(c, pos, (int)win.limit, floor);
      printf("%d %d %zu", win.query_size, nolim ? 2 : 0, spans.size());
      for (auto &sp : spans) {
        printf(" %d %d", sp[0], sp[1]);
        if (guard) {  // (the case is discarded)
          printf(" 0 0 0 0 0 1 0 0 0 0 0 0 0 0 0");
          continue;
        }
        roll_extend(c, *query, *ref, win, (int)i, (int)qwe, sp[0], sp[1]);
        if (guard) printf(" 1 0 0 0 0 0 0 0 0 0");
      }
      printf("\n");
    }
    printf("K %d %lld %lld %lld %lld %lld %lld\n", (int)guard, n_undo, n_false_undo, n_stop_len, n_stop_ratio, n_stop_overlap, n_at_end);
  }
  return 0;
}
"""
HIT_FIELDS = 17  # start, end, the roll's five, the hit's ten


def build_driver(tmp):
    src = os.path.join(tmp, "extend_driver.cc")
    exe = os.path.join(tmp, "extend_driver")
    with open(src, "w") as f:
        f.write(DRIVER)
    ref = W.REF
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-w", "-DNDEBUG", "-I" + ref, "-I" + os.path.join(ref, "src"), "-o", exe, src,
                           os.path.join(ref, "src", "hash.cc"), os.path.join(ref, "src", "sliding.cc"),
                           os.path.join(ref, "src", "globals.cc"), os.path.join(ref, "extern", "format.cc")])
    return exe


def run_driver(exe, cases):
    """[(windows, guard, counters)] of the cases."""
    lines = []
    for c in cases:
        head = [c["k"], c["w"], c["sl"], c["r_rc"], c["init_len"], c["same_genome"], c["uppercase_seeds"], c["same"], c["threshold"],
                repr(c["max_error"]), repr(c["max_edit_error"]), c["max_sd_size"], len(c["limit"])] + c["limit"]
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
            windows.append([qsz, flags, [[int(next(tok)) for _ in range(HIT_FIELDS)] for _ in range(nt)]])
        assert next(tok) == b"K"
        guard = int(next(tok))
        out.append((windows, guard, {name: int(next(tok)) for name in COUNTERS}))
    assert next(tok, None) is None
    return out


def one_genome_case(rng, it):
    """One genome against itself with tandem copies a little apart, so that a hit's query side grows into its reference side."""
    k, w = int(rng.integers(3, 6)), int(rng.integers(2, 5))
    unit = rng.integers(0, 4, int(rng.integers(40, 90)))
    parts = [rng.integers(0, 4, int(rng.integers(5, 30)))]
    for _ in range(int(rng.integers(3, 6))):
        parts += [W.mutate(rng, unit, 0.03), rng.integers(0, 4, int(rng.integers(0, 12)))]
    s = W.text(rng, np.concatenate(parts), lower=int(it % 3 == 0))
    return dict(name="one genome %d" % it, q=s, r="", r_rc=0, same=1, k=k, w=w, sl=int(it % 4 != 3), init_len=int(rng.choice([12, 20, 30])),
                same_genome=1, uppercase_seeds=int(it % 2), threshold=1 << 31, limit=W.table(300, float(rng.choice([0.1, 0.25, 0.4]))))


def two_sequences_case(rng, it):
    """A small case as the roll fixture's are, for the place of one that the guard discarded."""
    k, w = int(rng.integers(3, 6)), int(rng.integers(2, 5))
    qa, units = R.short_repeats(rng, int(rng.integers(150, 420)), int(rng.integers(8, 30)), int(rng.integers(4, 9)), 0.04)
    ra = np.concatenate([W.mutate(rng, units[int(rng.integers(0, 2))], 0.05) if rng.random() < 0.6 else rng.integers(0, 4, 9)
                         for _ in range(int(rng.integers(6, 16)))])
    return dict(name="small again %d" % it, q=W.text(rng, qa), r=W.text(rng, ra), r_rc=0, same=0, k=k, w=w, sl=int(it % 6 != 5),
                init_len=int(rng.choice([12, 20, 30, 45])), same_genome=0, uppercase_seeds=int(it % 2), threshold=1 << 31,
                limit=W.table(80, float(rng.choice([0.1, 0.25, 0.4]))))


def main():
    cases = R.make_cases(np.random.default_rng(20261020))  # the roll fixture's own
    rng = np.random.default_rng(20261103)
    cases += [one_genome_case(rng, it) for it in range(12)]
    for it, c in enumerate(cases):
        # the reference's defaults; a few of the small cases with a tighter size or ratio, so that every stop test ends rounds
        c.update(max_error=0.30, max_edit_error=0.15, max_sd_size=1 << 20)
        if c["k"] != 12 and it % 5 == 1:
            c["max_sd_size"] = int(rng.integers(40, 120))
        if c["k"] != 12 and it % 5 == 3:
            c["max_error"], c["max_edit_error"] = 0.25, 0.20
    redrawn = 0
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(tmp)
        todo = list(range(len(cases)))
        while todo:
            again = []
            for at, (windows, guard, counters) in zip(todo, run_driver(exe, [cases[at] for at in todo])):
                if guard:
                    redrawn += 1
                    assert cases[at]["k"] != 12, "the guard fired in a k = 12 case"
                    fresh = (one_genome_case if cases[at]["same_genome"] else two_sequences_case)(rng, 100 + redrawn)
                    fresh.update(name="%s (drawn again %d)" % (cases[at]["name"], redrawn),
                                 **{key: cases[at][key] for key in ("max_error", "max_edit_error", "max_sd_size")})
                    cases[at] = fresh
                    again.append(at)
                else:
                    cases[at].update(nq=len(windows), windows=windows, counters=counters)
            todo = again
    total = {name: sum(c["counters"][name] for c in cases) for name in COUNTERS}
    rows = [(c, w, t) for c in cases for w in c["windows"] for t in w[2]]
    hits = [(c, t) for c, w, t in rows if t[7] == 0]
    n_nolimit = sum(t[7] == NOLIMIT for c, w, t in rows)
    # a hit grew when a winnow range is wider than at its entry (the members, the roll's records)
    grew = sum(1 for c, t in hits if t[16] - t[15] > t[5] - t[4])
    k12 = [c for c in cases if c["k"] == 12]
    print("cases %d (drawn again: %d), intervals %d, hits %d (k = 12: %d), grown %d, beyond the table %d; counters %s"
          % (len(cases), redrawn, len(rows), len(hits), sum(1 for c, t in hits if c["k"] == 12), grew, n_nolimit, total))
    assert all(v > 0 for v in total.values()), total
    assert 5 * grew >= len(hits) and n_nolimit > 0
    assert any(c["same_genome"] for c in k12) and any(c["r_rc"] for c in k12)
    path = os.path.join(ROOT, "tests", "golden", "search_extend_kat.json.gz")
    blob = json.dumps(dict(source="reference SlidingMap and Index, the roll of src/search.cc:274-314 and extend() of src/search.cc:95-259 "
                                  "via the driver of tests/golden/make_golden_search_extend.py", redrawn=redrawn, cases=cases),
                      separators=(",", ":")).encode()
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(blob)
    size = os.path.getsize(path)
    print("wrote %s: %d cases, %d bytes (%d uncompressed)" % (path, len(cases), size, len(blob)))
    assert size <= 300000, size


if __name__ == "__main__":
    sys.exit(main())
