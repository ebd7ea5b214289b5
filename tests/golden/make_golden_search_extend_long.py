#!/usr/bin/env python3
"""Generates tests/golden/search_extend_long_kat.json.gz: a handful of cases in which the REFERENCE's extend() grows a winnow
range by more than SDF_EXTEND_MAX_GROW = 1,792 records at some end -- the growths the long form of the extension answers on the
device (sdf_search_extend_long_device) and on which sdf_search_extend_host, its truth, was not pinned so far.  The driver, the
guard and the format of a case are those of make_golden_search_extend.py (build_driver / run_driver are imported, not copied):
the reference's own SlidingMap and Index; a case that reaches a spot the reference leaves undefined is drawn again.

A case is two sequences of some kilobases, one a mutated copy of the other -- or one genome that holds both copies --, soft-masked
but for a short island: with uppercase_seeds only the windows at the island have intervals, so the fixture stays small, while
the extension, which adds records whatever their case, runs from there to the sequences' ends, thousands of records away (k and
w are small: a record every two or three bases).  Needs /root/reference (build container only); the fixture is data."""
import gzip
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
import make_golden_search_extend as X  # noqa: E402
import make_golden_search_windows as W  # noqa: E402

MAX_GROW = 1792


def masked(a, islands):
    """Codes as characters, lowercase but for the islands [(at, length) ...]."""
    s = W.LETTERS[a] | 0x20
    for at, ln in islands:
        s[at:at + ln] &= 0xDF
    return s.tobytes().decode()


def two_sequences_case(rng, it):
    k, w = [(3, 2), (4, 2), (5, 3)][it % 3]
    n = int(rng.integers(6500, 7500)) * (w + 1) // 3
    at = int(rng.integers(300, 900)) if it % 2 else n - int(rng.integers(300, 900))  # the long growth to the right, or to the left
    qa = rng.integers(0, 4, n)
    ra = qa.copy()
    hit = rng.random(n) < 0.02
    hit[at - 40:at + 80] = False
    ra[hit] = (ra[hit] + rng.integers(1, 4, int(hit.sum()))) % 4
    island = [(at, int(rng.integers(14, 22)))]
    return dict(name="two sequences %d" % it, q=masked(qa, island), r=masked(ra, island), r_rc=0, same=0, k=k, w=w, sl=1,
                init_len=int(rng.choice([12, 20, 30])), same_genome=0, uppercase_seeds=1, threshold=1 << 31,
                limit=W.table(2 * 4 ** k + 40, float(rng.choice([0.2, 0.3]))))


def one_genome_case(rng, it):
    """Two copies of one unit a little apart in one sequence; the island lies early in the unit, so both copies grow to the right
    by the unit's length."""
    k, w = [(3, 2), (4, 2)][it % 2]
    unit = rng.integers(0, 4, int(rng.integers(6000, 6600)))
    copy = unit.copy()
    at = int(rng.integers(200, 500))
    hit = rng.random(len(unit)) < 0.02
    hit[at - 40:at + 80] = False
    copy[hit] = (copy[hit] + rng.integers(1, 4, int(hit.sum()))) % 4
    head, gap = int(rng.integers(50, 200)), int(rng.integers(150, 400))
    a = np.concatenate([rng.integers(0, 4, head), unit, rng.integers(0, 4, gap), copy, rng.integers(0, 4, 60)])
    ln = int(rng.integers(14, 22))
    s = masked(a, [(head + at, ln), (head + len(unit) + gap + at, ln)])
    return dict(name="one genome %d" % it, q=s, r="", r_rc=0, same=1, k=k, w=w, sl=1, init_len=int(rng.choice([12, 20])), same_genome=1,
                uppercase_seeds=1, threshold=1 << 31, limit=W.table(2 * 4 ** k + 40, float(rng.choice([0.2, 0.3]))))


def growth(t):
    """The records by which the reference side of a hit row grew beyond the roll's winnow range, at its wider end."""
    return max(t[4] - t[15], t[16] - t[5])


def main():
    rng = np.random.default_rng(20261120)
    makers = [two_sequences_case, two_sequences_case, two_sequences_case, one_genome_case, one_genome_case]
    cases, redrawn = [], 0
    with tempfile.TemporaryDirectory() as tmp:
        exe = X.build_driver(tmp)
        for it, make in enumerate(makers):
            while True:
                c = make(rng, it)
                c.update(max_error=0.30, max_edit_error=0.15, max_sd_size=1 << 20)
                (windows, guard, counters), = X.run_driver(exe, [c])
                hits = [t for w in windows for t in w[2] if t[7] == 0]
                if not guard and hits and max(growth(t) for t in hits) > MAX_GROW:
                    break
                redrawn += 1  # the guard fired, or no growth passed the short form's cap
                assert redrawn < 50
            c.update(nq=len(windows), windows=windows, counters=counters)
            cases.append(c)
    rows = [t for c in cases for w in c["windows"] for t in w[2]]
    long_hits = [t for t in rows if t[7] == 0 and growth(t) > MAX_GROW]
    print("cases %d (drawn again: %d), intervals %d, hits %d, of them grown beyond %d records: %d (the widest: %d)"
          % (len(cases), redrawn, len(rows), sum(t[7] == 0 for t in rows), MAX_GROW, len(long_hits), max(growth(t) for t in long_hits)))
    assert all(any(t[7] == 0 and growth(t) > MAX_GROW for w in c["windows"] for t in w[2]) for c in cases)
    path = os.path.join(ROOT, "tests", "golden", "search_extend_long_kat.json.gz")
    blob = json.dumps(dict(source="reference SlidingMap and Index, the roll of src/search.cc:274-314 and extend() of src/search.cc:95-259 "
                                  "via the driver of tests/golden/make_golden_search_extend.py; growths beyond 1,792 records",
                           redrawn=redrawn, cases=cases), separators=(",", ":")).encode()
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(blob)
    size = os.path.getsize(path)
    print("wrote %s: %d cases, %d bytes (%d uncompressed)" % (path, len(cases), size, len(blob)))
    assert size <= 95000, size


if __name__ == "__main__":
    sys.exit(main())
