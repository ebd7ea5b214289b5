#!/usr/bin/env python3
"""Generates tests/golden/minimizers_kat.json.gz: sequences and what the REFERENCE's own get_minimizers and Index::Index
(src/hash.cc:53-141) answer for them.  The small driver below is ours; it includes the reference's hash.h and is compiled
here, into a temporary directory, against the reference's unmodified src/hash.cc, src/globals.cc and extern/format.cc where
they lie.  Needs /root/reference (build container only); the fixture is data: inputs and expected outputs.

A case is {name, seq, k, w, sl (separate_lowercase), rc}.  rc = 1: the reference was given Sequence(name, seq, true), so the
lists are in the coordinates of the reverse complement (rc is src/util.cc:43, which needs Boost to build: the driver states
it again with the reference's rev_dna).  Small cases hold `minimizers` [[hash, loc, status]], `n_groups`, `threshold` and
`groups` [[status, hash, [locs]]] in ascending (status, hash) order -- the reference's map is unordered, the order is the
driver's.  The few LONG cases hold the counts and sha256 digests of the same lists as little-endian int32 triples
(hash, loc, status; the groups flattened in their order), because only a sequence of 100,000 minimizers and more has
ignore >= 1 (ignore = int(n * 0.001 / 100)) and lets the threshold leave 2^31: they are built from repeats, which compress."""
import gzip
import hashlib
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
#include <cstdio>
#include <iostream>
#include <map>
#include <memory>
#include <string>
#include <vector>
#include "common.h"
#include "hash.h"
using namespace std;
vector<Minimizer> get_minimizers(const string &s, int kmer_size, const int window_size, bool separate_lowercase);  // src/hash.cc:53
// src/util.cc does not build without Boost: the one function of it that Sequence's constructor calls
string rc(const string &s) {
  string r(s.size(), 'N');
  for (size_t i = 0; i < s.size(); i++) r[i] = rev_dna(s[s.size() - 1 - i]);
  return r;
}
int main() {
  int k, w, sl, is_rc;
  size_t len;
  while (cin >> k >> w >> sl >> is_rc >> len) {
    string s;
    if (len) cin >> s;
    if (s.size() != len) return 2;
    auto seq = make_shared<Sequence>("case", s, is_rc != 0);
    auto direct = get_minimizers(seq->seq, k, w, sl != 0);
    Index idx(seq, k, w, sl != 0);
    if (!(direct.size() == idx.minimizers.size() && equal(direct.begin(), direct.end(), idx.minimizers.begin()))) return 3;
    printf("M %zu\n", direct.size());
    for (auto &m : direct) printf("%u %d %d\n", m.hash.hash, m.loc, (int)m.hash.status);
    map<pair<int, unsigned>, vector<int>> groups;
    for (auto &g : idx.index) groups[{(int)g.first.status, g.first.hash}] = vector<int>(g.second.begin(), g.second.end());
    printf("I %zu %u\n", groups.size(), idx.threshold);
    for (auto &g : groups) {
      printf("%d %u %zu", g.first.first, g.first.second, g.second.size());
      for (int loc : g.second) printf(" %d", loc);
      printf("\n");
    }
  }
  return 0;
}
"""


def build_driver(tmp):
    src = os.path.join(tmp, "minim_driver.cc")
    exe = os.path.join(tmp, "minim_driver")
    with open(src, "w") as f:
        f.write(DRIVER)
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-w", "-I" + REF, "-I" + os.path.join(REF, "src"), "-o", exe, src,
                           os.path.join(REF, "src", "hash.cc"), os.path.join(REF, "src", "globals.cc"),
                           os.path.join(REF, "extern", "format.cc")])
    return exe


def run_driver(exe, cases):
    text = "".join("%d %d %d %d %d %s\n" % (c["k"], c["w"], c["sl"], c["rc"], len(c["seq"]), c["seq"]) for c in cases)
    tok = iter(subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, check=True).stdout.split())
    out = []
    for _ in cases:
        assert next(tok) == b"M"
        mins = [[int(next(tok)), int(next(tok)), int(next(tok))] for _ in range(int(next(tok)))]
        assert next(tok) == b"I"
        n_groups, threshold = int(next(tok)), int(next(tok))
        groups = []
        for _ in range(n_groups):
            st, h, cnt = int(next(tok)), int(next(tok)), int(next(tok))
            groups.append([st, h, [int(next(tok)) for _ in range(cnt)]])
        out.append((mins, n_groups, threshold, groups))
    assert next(tok, None) is None
    return out


def digest(rows):
    return hashlib.sha256(np.asarray(rows, dtype="<i4").reshape(-1, 3).tobytes()).hexdigest()


def flat_groups(groups):
    return [(h, loc, st) for st, h, locs in groups for loc in locs]


def small_cases(rng):
    cases = []

    def add(name, seq, k, w, sl=1, rc=0):
        assert len(seq) <= 400
        cases.append(dict(name=name, seq=seq, k=k, w=w, sl=sl, rc=rc))

    def rnd(n, alphabet="ACGT"):
        return "".join(alphabet[i] for i in rng.integers(0, len(alphabet), n))

    # every nk in {0, 1, w - 1, w, w + 1, w + 2}, and len < k
    for k, w in ((12, 16), (1, 1), (2, 5), (15, 3), (12, 1), (5, 16)):
        for nk in sorted({0, 1, w - 1, w, w + 1, w + 2}):
            for rc in (0, 1):
                add("nk=%d k=%d w=%d" % (nk, k, w), rnd(nk + k - 1, "ACGTacgt"), k, w, 1, rc)
        for ln in sorted({0, 1, k - 1}):
            if ln < k:
                add("len=%d < k=%d" % (ln, k), rnd(ln), k, w)
    for k in (1, 2, 12, 15):
        for w in (1, 2, 16, 40):
            for rc in (0, 1):
                add("random k=%d w=%d" % (k, w), rnd(int(rng.integers(100, 400))), k, w, 1, rc)
                add("random, few letters k=%d w=%d" % (k, w), rnd(int(rng.integers(100, 400)), "AAC"), k, w, 1, rc)
    # poly-A: every position >= w is a minimizer
    for k, w, n in ((12, 16, 200), (1, 1, 50), (15, 7, 399), (2, 40, 100)):
        for ch in "Aa":
            add("poly-%s k=%d w=%d" % (ch, k, w), ch * n, k, w, 1, 0)
            add("poly-%s k=%d w=%d" % (ch, k, w), ch * n, k, w, 0, 1)
    # strictly rising and strictly falling hashes (k = 1, 2: a monotone run of characters; longer k: A..AC..CG..GT..T)
    for k, w in ((1, 2), (2, 3), (12, 16), (12, 5)):
        rise = "A" * 90 + "C" * 90 + "G" * 90 + "T" * 90
        add("rising k=%d w=%d" % (k, w), rise, k, w)
        add("falling k=%d w=%d" % (k, w), rise[::-1], k, w)
        add("rising, then its mirror k=%d w=%d" % (k, w), rise[:150] + rise[:150][::-1], k, w, 1, 1)
    # runs of N shorter and longer than k
    for k, w in ((12, 16), (5, 4), (15, 1)):
        for run in (1, k - 1, k, k + 1, 3 * k):
            for n_char in "Nn":
                s = rnd(120, "ACGTacgt")
                at = int(rng.integers(20, 60))
                add("N run of %d (%s) k=%d w=%d" % (run, n_char, k, w), s[:at] + n_char * run + s[at:], k, w, 1, int(rng.integers(0, 2)))
    # mixed case with separate_lowercase 0 and 1: blocks of either case longer and shorter than k
    for k, w in ((12, 16), (2, 1), (15, 8), (5, 30)):
        for it in range(4):
            s = ""
            while len(s) < 350:
                blk = rnd(int(rng.integers(1, 3 * k + 4)))
                s += blk.lower() if rng.random() < 0.5 else blk
            for sl in (0, 1):
                for rc in (0, 1):
                    add("mixed case k=%d w=%d" % (k, w), s[:380], k, w, sl, rc)
    # letters that are not ACGT: R is no N forward and an N after the reverse complement
    for k, w in ((12, 16), (3, 2), (15, 16)):
        for it in range(4):
            s = list(rnd(300, "ACGTacgt"))
            for at in rng.choice(300, 12, replace=False):
                s[int(at)] = "RrYyKMSW-*."[int(rng.integers(0, 11))]
            for sl in (0, 1):
                for rc in (0, 1):
                    add("other letters k=%d w=%d" % (k, w), "".join(s), k, w, sl, rc)
    # tandem repeats: equal keys a window apart and closer
    for k, w in ((12, 16), (4, 16), (12, 3)):
        for period in (1, 2, 3, w, w + 1, w - 1):
            unit = rnd(max(period, 1))
            add("period %d k=%d w=%d" % (period, k, w), (unit * 400)[:390], k, w, 1, int(rng.integers(0, 2)))
    return cases


def long_cases(rng):
    def repeats(total, unit_len, every):
        unit = rng.integers(0, 4, unit_len)
        a = np.tile(unit, total // unit_len + 1)[:total].copy()
        where = np.arange(every, total, every)
        a[where] = (a[where] + 1) % 4
        return a

    def text(a, lower_from=None):
        s = np.frombuffer(b"ACGT", np.uint8)[a].copy()
        if lower_from is not None:
            s[lower_from:] |= 0x20
        return s

    cases = []
    # k = 12, w = 16 (what the pipeline runs): 2 M characters of a 5,000-character unit; 3,000 A in a row make ONE largest group
    s = text(repeats(2000000, 5000, 1013))
    s[300000:303000] = ord("A")
    cases.append(dict(name="long: repeats and one poly-A run, k=12 w=16", seq=s.tobytes().decode(), k=12, w=16, sl=1, rc=0))
    # w = 2: two runs of different lengths, so that the walk takes two sizes (ignore = 2)
    s = text(repeats(600000, 3000, 701), lower_from=400000)
    s[50000:54000] = ord("A")
    s[120000:122500] = ord("C")
    s[250000:250040] = ord("N")
    cases.append(dict(name="long: two runs, k=12 w=2", seq=s.tobytes().decode(), k=12, w=2, sl=1, rc=0))
    cases.append(dict(name="long: two runs, k=12 w=2, reversed", seq=s.tobytes().decode(), k=12, w=2, sl=1, rc=1))
    # the same characters where no group stands out: the threshold stays
    s = text(repeats(330000, 3000, 701))
    cases.append(dict(name="long: repeats alone, k=15 w=1", seq=s.tobytes().decode(), k=15, w=1, sl=0, rc=0))
    return cases


def main():
    rng = np.random.default_rng(20261018)
    small, big = small_cases(rng), long_cases(rng)
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(tmp)
        for c, (mins, n_groups, threshold, groups) in zip(small, run_driver(exe, small)):
            c.update(minimizers=mins, n_groups=n_groups, threshold=threshold, groups=groups)
        for c, (mins, n_groups, threshold, groups) in zip(big, run_driver(exe, big)):
            c.update(n_minimizers=len(mins), minimizers_sha256=digest(mins), n_groups=n_groups, threshold=threshold,
                     groups_sha256=digest(flat_groups(groups)))
    assert 200 <= len(small) <= 900, len(small)
    moved = [c for c in big if c["threshold"] != 1 << 31]
    assert len(moved) >= 2 and all(c["n_minimizers"] >= 100000 for c in big), [(c["n_minimizers"], c["threshold"]) for c in big]
    assert any(c["threshold"] == 1 << 31 for c in big)
    assert all(c["threshold"] == 1 << 31 for c in small)
    for c in small:
        nk = len(c["seq"]) - c["k"] + 1
        assert (len(c["minimizers"]) == 0) == (nk <= c["w"]), c["name"]
    path = os.path.join(ROOT, "tests", "golden", "minimizers_kat.json.gz")
    blob = json.dumps(dict(source="reference get_minimizers / Index::Index (src/hash.cc:53-141) via the driver of "
                                  "tests/golden/make_golden_minimizers.py", cases=small, long_cases=big),
                      separators=(",", ":")).encode()
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(blob)
    print("wrote %s: %d + %d cases, %d bytes; long: %s" % (path, len(small), len(big), os.path.getsize(path),
                                                          [(c["n_minimizers"], c["n_groups"], c["threshold"]) for c in big]))


if __name__ == "__main__":
    sys.exit(main())
