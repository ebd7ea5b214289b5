#!/usr/bin/env python3
"""Generates tests/golden/search_filter_kat.json.gz: pools of characters, pairs of their ranges and what the REFERENCE's own
filter() (src/filter.cc) answers for each pair.  src/filter.h includes search.h, which does not build here (Boost), so the
generator copies src/filter.cc into a temporary directory next to a three-line filter.h of its own -- common.h and the
declaration of filter() -- and compiles it there with -DNDEBUG (below minqg 10 the reference then answers instead of aborting)
together with src/globals.cc and extern/format.cc where they lie; the directory is deleted afterwards.  The driver below is in
our own words: it sets Globals::Search::* per call, builds a reverse strand with the reference's rev_dna, calls filter() and
parses the failure strings.  Needs /root/reference (build container only); the fixture is data.

filter() prints nothing when a pair passes and hides dist behind an uppercase failure, so every pair is called four times:
as it is (the verdict); with MIN_UPPERCASE above both lengths (q_up, r_up); with MIN_UPPERCASE 0, MAX_ERROR -10 and the other
two 0, where minqg = 11 l - 4 exceeds every dist (dist); and as poly-A against poly-C of the pair's l with MIN_UPPERCASE 0,
which prints minqg whenever it is above 0.  A pair whose dist or minqg stays hidden (l = 0; minqg <= 0) is recorded by its
verdict alone and counted: at most 10 % of the pairs.

A case is {name, pool, params, tasks, records, counters}: a task is [q_off, r_off, q_len, r_len, flags], a record
[q_up, r_up, dist, minqg, flags] or, verdict only, [q_up, r_up, null, null, flags & 3].  A roll case also names the case of
search_roll_kat.json.gz it was built on, allow_extend and where its sequences lie in the pool.  Its TASKS ARE NOT REFERENCE
OUTPUT: src/search.cc does not build here, so which ranges the reference would filter -- the final-versus-best position of
search.cc:337-338 among them -- is tests/filter_model.py's reading of search.cc:274-338 applied to the fixture's roll records;
the records of those tasks are the reference's filter() like every other.  sweep: per parameter set the [l, minqg] of every l
from 1 to 2,000 and of 200 lengths up to 2^20 (minqg null where the reference printed nothing: minqg <= 0).

`--dump-cases FILE [name ...]` needs no reference: it writes cases of the committed fixture (default: the first pairs case and the
first roll case) in the layout profiles/search_filter_host_check.cc reads, the records expected by tests/filter_model.py, which
tests/test_search_filter_cpu.py holds against the fixture."""
import gzip
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = os.environ.get("SEDEF_REFERENCE", "/root/reference")

import filter_model as F  # noqa: E402

COUNTERS = ("passes", "upper_fail", "qgram_fail", "short", "rc_sides", "short_sides", "final_differs")
PARAM_SETS = [dict(F.DEFAULTS), dict(min_uppercase=12, max_error=0.25, max_edit_error=0.10, gap_frequency=0.005),
              dict(min_uppercase=12, max_error=0.30, max_edit_error=0.15, gap_frequency=0.0)]

FILTER_H = """#pragma once
#include "common.h"
std::pair<bool, std::string> filter(const std::string &q, int q_pos, int q_end, const std::string &r, int r_pos, int r_end);
"""

DRIVER = r"""
#include <algorithm>
#include <cstdio>
#include <iostream>
#include <string>
#include "filter.h"
using namespace std;

static int g_up;
static double g_me, g_mee, g_gf;
static void params(int up, double me, double mee, double gf) {
  Globals::Search::MIN_UPPERCASE = up, Globals::Search::MAX_ERROR = me, Globals::Search::MAX_EDIT_ERROR = mee,
  Globals::Search::GAP_FREQUENCY = gf;
}
static string strand(const string &s, int rc) {
  if (!rc) return s;
  string o(s.rbegin(), s.rend());
  for (auto &c : o) c = rev_dna(c);
  return o;
}
static string whole(const string &q, const string &r) { return filter(q, 0, (int)q.size(), r, 0, (int)r.size()).second; }

int main() {
  string op;
  while (cin >> op) {
    if (op == "P") {
      cin >> g_up >> g_me >> g_mee >> g_gf;
    } else if (op == "S") {  // minqg of l, from a pair without a common gram
      int l;
      cin >> l;
      params(0, g_me, g_mee, g_gf);
      int d, m;
      const string s = whole(string(l, 'A'), string(l, 'C'));
      if (sscanf(s.c_str(), "q-grams %d < %d", &d, &m) == 2 && d == 0) printf("%d\n", m);
      else printf("-\n");
    } else if (op == "F") {
      int qrc, rrc;
      string qs, rs;
      cin >> qrc >> rrc >> qs >> rs;  // (each behind a dot: a side may be empty)
      const string q = strand(qs.substr(1), qrc), r = strand(rs.substr(1), rrc);
      const int l = (int)max(q.size(), r.size());
      int a, b, c;
      params(g_up, g_me, g_mee, g_gf);
      string s = whole(q, r);
      const int verdict = s.empty() ? 0 : s[0] == 'u' ? 1 : 2;
      params(l + 1, g_me, g_mee, g_gf);
      s = whole(q, r);
      if (sscanf(s.c_str(), "upper (%d, %d) < %d", &a, &b, &c) != 3) return 2;
      printf("%d %d %d", verdict, a, b);
      params(0, -10.0, 0.0, 0.0);
      s = whole(q, r);
      if (sscanf(s.c_str(), "q-grams %d < %d", &a, &b) == 2) printf(" %d", a);
      else printf(" -");
      params(0, g_me, g_mee, g_gf);
      s = whole(string(l, 'A'), string(l, 'C'));
      if (sscanf(s.c_str(), "q-grams %d < %d", &a, &b) == 2 && a == 0) printf(" %d\n", b);
      else printf(" -\n");
    }
  }
  return 0;
}
"""


def build_driver(tmp):
    shutil.copy(os.path.join(REF, "src", "filter.cc"), os.path.join(tmp, "filter.cc"))
    with open(os.path.join(tmp, "filter.h"), "w") as f:
        f.write(FILTER_H)
    with open(os.path.join(tmp, "filter_driver.cc"), "w") as f:
        f.write(DRIVER)
    exe = os.path.join(tmp, "filter_driver")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-w", "-DNDEBUG", "-I" + tmp, "-I" + REF, "-I" + os.path.join(REF, "src"), "-o", exe,
                           os.path.join(tmp, "filter_driver.cc"), os.path.join(tmp, "filter.cc"), os.path.join(REF, "src", "globals.cc"),
                           os.path.join(REF, "extern", "format.cc")])
    return exe


def run(exe, lines):
    return subprocess.run([exe], input=("\n".join(lines) + "\n").encode(), stdout=subprocess.PIPE, check=True).stdout.decode().split("\n")[:-1]


def param_line(P):
    return "P %d %r %r %r" % (P["min_uppercase"], P["max_error"], P["max_edit_error"], P["gap_frequency"])


def reference_records(exe, c):
    """The case's records from the reference; its counters (final_differs stays with the caller)."""
    pool, lines = c["pool"], [param_line(c["params"])]
    for qo, ro, ql, rl, fl in c["tasks"]:
        lines.append("F %d %d .%s .%s" % (bool(fl & F.Q_RC), bool(fl & F.R_RC), pool[qo:qo + ql], pool[ro:ro + rl]) if not fl & F.SKIP else "")
    out = iter(run(exe, [x for x in lines if x]))
    n = dict.fromkeys(COUNTERS, 0)
    n["verdict_only"] = 0
    records = []
    for qo, ro, ql, rl, fl in c["tasks"]:
        if fl & F.SKIP:
            records.append([0, 0, 0, 0, F.SKIPPED])
            continue
        verdict, q_up, r_up, dist, m = next(out).split()
        flags = int(verdict)
        n[("passes", "upper_fail", "qgram_fail")[flags]] += 1
        n["rc_sides"] += bool(fl & F.Q_RC) + bool(fl & F.R_RC)
        n["short_sides"] += (ql < 5) + (rl < 5)
        if dist == "-" or m == "-":
            n["verdict_only"] += 1
            records.append([int(q_up), int(r_up), None, None, flags])
            continue
        if int(m) < 10:
            flags |= F.SHORT
            n["short"] += 1
        records.append([int(q_up), int(r_up), int(dist), int(m), flags])
    assert next(out, None) is None
    return records, n


LETTERS = np.frombuffer(b"ACGT", np.uint8)


def mutate(rng, a, rate):
    """Substitutions at `rate`, and a few short deletions and insertions."""
    a = a.copy()
    hit = rng.random(len(a)) < rate
    a[hit] = (a[hit] + rng.integers(1, 4, int(hit.sum()))) % 4
    for _ in range(int(rng.integers(0, 4))):
        at, ln = int(rng.integers(0, max(1, len(a) - 8))), int(rng.integers(1, 6))
        a = np.concatenate([a[:at], a[at + ln:]]) if rng.random() < 0.5 else np.concatenate([a[:at], rng.integers(0, 4, ln), a[at:]])
    return a


def text(rng, codes, lower=0.0, n_runs=0, others=0, letters=LETTERS):
    """Codes as characters: a share of soft-masked stretches, runs of N / n, single other letters."""
    s = letters[codes].copy()
    done = 0
    while len(s) > 20 and done < lower * len(s):
        at, ln = int(rng.integers(0, len(s) - 8)), int(rng.integers(8, max(9, len(s) // 3)))
        s[at:at + ln] |= 0x20
        done += ln
    for _ in range(n_runs if len(s) > 30 else 0):
        at, ln = int(rng.integers(0, len(s) - 10)), int(rng.integers(1, 25))
        s[at:at + ln] = ord("N") if rng.random() < 0.5 else ord("n")
    for _ in range(others if len(s) > 4 else 0):
        s[int(rng.integers(0, len(s)))] = int(rng.choice(list(b"RxYkMw")))
    return s.tobytes().decode()


def pair_cases(rng):
    cases = []
    for ci in range(12):
        P = dict(PARAM_SETS[ci % 3], min_uppercase=int(rng.choice([0, 12, 12, 40, 250])))
        pool, tasks = "", []

        def put(s):
            nonlocal pool
            pool += "acgtN"[:int(rng.integers(0, 6))] + s
            return len(pool) - len(s), len(s)

        for it in range(22):
            kind = ("related", "related", "related", "unrelated", "disjoint", "runs", "tiny")[int(rng.integers(0, 7))]
            n = int(rng.choice([30, 90, 180, 260, 420, 700, 700, 1000, 1600]) * rng.uniform(0.7, 1.2))
            lower = float(rng.choice([0, 0, 0.2, 0.6, 1.5]))
            if kind == "related":
                a = rng.integers(0, 4, n)
                q = put(text(rng, a, lower, int(rng.integers(0, 2)), int(rng.integers(0, 3))))
                r = put(text(rng, mutate(rng, a, float(rng.uniform(0.05, 0.30))), lower, int(rng.integers(0, 2)), int(rng.integers(0, 3))))
            elif kind == "unrelated":
                q = put(text(rng, rng.integers(0, 4, n), lower, 1, 1))
                r = put(text(rng, rng.integers(0, 4, int(n * rng.uniform(0.5, 1.5))), lower, 0, 2))
            elif kind == "disjoint":
                q = put(text(rng, rng.integers(0, 2, n), lower, letters=np.frombuffer(b"ACAC", np.uint8)))
                r = put(text(rng, rng.integers(0, 2, n), lower, letters=np.frombuffer(b"GTGT", np.uint8)))
            elif kind == "runs":  # homopolymer and dinucleotide runs, some of them shared
                unit = [rng.integers(0, 4, 1), rng.integers(0, 4, 2), rng.integers(0, 4, 1)]
                parts = [np.tile(unit[int(rng.integers(0, 3))], int(rng.integers(10, 150))) for _ in range(4)] + [rng.integers(0, 4, n // 4)]
                a = np.concatenate([parts[x] for x in rng.permutation(len(parts))])
                q = put(text(rng, a, lower, 0, 1))
                r = put(text(rng, mutate(rng, a, 0.08), lower, 1, 0))
            else:  # sides shorter than 5, an empty one
                q = put(text(rng, rng.integers(0, 4, int(rng.integers(0, 7)))))
                r = put(text(rng, rng.integers(0, 4, int(rng.choice([0, 3, 4, 5, 6, 200])))))
            flags = int(rng.choice([0, 0, 0, F.Q_RC, F.R_RC, F.Q_RC | F.R_RC]))
            if kind == "related" and flags in (F.Q_RC, F.R_RC):  # one side turned round: the pair is related when the pool holds it reversed
                lo, ln = r if flags == F.R_RC else q
                pool = pool[:lo] + F.side(pool.encode(), lo, ln, True).tobytes().decode() + pool[lo + ln:]
            tasks.append([q[0], r[0], q[1], r[1], flags])
        cases.append(dict(name="pairs %d" % ci, pool=pool, params=P, tasks=tasks))
    return cases


def roll_cases():
    """Two or three cases of search_roll_kat.json.gz through the task builder's rules (tests/filter_model.py), both values of
    allow_extend."""
    import test_search_roll_cpu as T
    kat = T.load_fixture()
    cases = []
    for name in ("k12 0", "k12 reversed reference", "small 3"):
        c = next(x for x in kat["cases"] if x["name"] == name)
        q, windows, first, intervals, r, len_r, init_len, limit = T.case_inputs(c)
        rolls = T.case_expected(c)
        pool = "ttgacca" + c["q"] + "NNcat"
        q_off, r_off = 7, len(pool)
        pool += c["r"] + "ac"
        for allow_extend in (1, 0):
            tasks = F.filter_tasks(q, windows, first, intervals, rolls, len(c["q"]), len_r, init_len, q_off, 0, r_off, c["r_rc"], allow_extend)
            P = dict(F.DEFAULTS) if c["k"] == 12 else dict(F.DEFAULTS, min_uppercase=4, max_error=0.2, max_edit_error=0.05)
            cases.append(dict(name="roll %s allow_extend %d" % (name, allow_extend), roll_case=name, allow_extend=allow_extend, q_off=q_off,
                              r_off=r_off, pool=pool, params=P,
                              tasks=[[int(t["q_off"]), int(t["r_off"]), int(t["q_len"]), int(t["r_len"]), int(t["flags"])] for t in tasks]))
    for a, b in zip(cases[0::2], cases[1::2]):
        a["final_differs"] = sum(x != y for x, y in zip(a["tasks"], b["tasks"]))
        b["final_differs"] = 0
    return cases


def sweep(exe):
    grid = np.unique(np.round(np.geomspace(2001, 1 << 20, 200)).astype(np.int64)).tolist()
    grid = (grid + list(range(1 << 20, (1 << 20) - 200, -1)))[:200]
    lengths = list(range(1, 2001)) + sorted(set(grid))
    assert len(lengths) == 2200 and lengths[-1] == 1 << 20
    out = []
    for P in PARAM_SETS:
        got = run(exe, [param_line(P)] + ["S %d" % l for l in lengths])
        out.append(dict(params=P, minqg=[[l, None if g == "-" else int(g)] for l, g in zip(lengths, got)]))
    return out


def dump_cases(path, names):
    import struct
    with gzip.open(os.path.join(ROOT, "tests", "golden", "search_filter_kat.json.gz"), "rb") as f:
        cases = json.loads(f.read().decode())["cases"]
    names = names or [cases[0]["name"], next(c["name"] for c in cases if "roll_case" in c)]
    with open(path, "wb") as f:
        for c in (c for c in cases if c["name"] in names):
            pool, P = c["pool"].encode(), c["params"]
            tasks = np.array([tuple(t) + (0,) for t in c["tasks"]], F.TASK)
            f.write(struct.pack("<Q", len(pool)) + pool + struct.pack("<Q", len(tasks)) + tasks.tobytes())
            f.write(struct.pack("<iiddd", P["min_uppercase"], 0, P["max_error"], P["max_edit_error"], P["gap_frequency"]))
            f.write(F.filter_pairs(pool, tasks, **P).tobytes())
            print("%s: %d tasks" % (c["name"], len(tasks)))


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--dump-cases":
        return dump_cases(sys.argv[2], sys.argv[3:])
    rng = np.random.default_rng(20261021)
    cases = pair_cases(rng) + roll_cases()
    tmp = tempfile.mkdtemp()
    try:
        exe = build_driver(tmp)
        for c in cases:
            c["records"], n = reference_records(exe, c)
            n["final_differs"] = c.pop("final_differs", 0)
            c["counters"] = n
        sw = sweep(exe)
    finally:
        shutil.rmtree(tmp)
    total = {name: sum(c["counters"][name] for c in cases) for name in COUNTERS + ("verdict_only",)}
    pairs = sum(len(c["tasks"]) for c in cases)
    print("pairs %d, counters %s" % (pairs, total))
    assert all(total[name] > 0 for name in COUNTERS), total
    assert 10 * total["verdict_only"] <= pairs, (total["verdict_only"], pairs)
    path = os.path.join(ROOT, "tests", "golden", "search_filter_kat.json.gz")
    blob = json.dumps(dict(source="reference filter() (src/filter.cc) via the driver of tests/golden/make_golden_search_filter.py",
                           cases=cases, sweep=sw), separators=(",", ":")).encode()
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(blob)
    size = os.path.getsize(path)
    print("wrote %s: %d cases, %d bytes (%d uncompressed)" % (path, len(cases), size, len(blob)))
    assert size <= 300000, size


if __name__ == "__main__":
    sys.exit(main())
