"""The case tables of the pair-recall tests (test_pair_recall_cpu.py, test_gpu_pair_recall.py): name -> (gold rows, found rows,
call flags).  Every table asserts, against the model, that it reaches the edge it is there for.  Rows are
(chr1, start1, end1, chr2, start2, end2, flags); three chromosomes, 0 .. 2.

The constants the tables are built against:
  CAP     SDF_RECALL_CAP as include/sedef_hip.h exports it: the clipped intervals per end recall_kernel keeps in LDS
  WALK    64: the candidates a wavefront of recall_kernel tests a round
  the sort window: a gold end [s, e) looks at the found ends that start in (s - L, e), L the longest found end of the call
  (sdf_kernels.h: the candidates); its two seams are a start of s - L + 1 / s - L and of e - 1 / e."""
import functools
import os
import re

import numpy as np

import recall_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = int(re.search(r"#define SDF_RECALL_CAP (\d+)", open(os.path.join(ROOT, "include", "sedef_hip.h")).read()).group(1))
WALK = 64
STEP = 100000  # units of a table lie this far apart: no unit's records reach another's


def shift(row, k):
    r = list(row)
    r[1] += k * STEP
    r[2] += k * STEP
    r[4] += k * STEP
    r[5] += k * STEP
    return tuple(r)


def units(specs):
    """[(gold row, [found rows])] -> (gold, found): unit k moved by k * STEP on both ends."""
    gold, found = [], []
    for k, (g, fs) in enumerate(specs):
        gold.append(shift(g, k))
        found += [shift(f, k) for f in fs]
    return gold, found


G = (0, 1000, 2000, 1, 5000, 6000, 0)  # the gold record most units use
IN2 = (5400, 5600)                     # a side-2 partner well inside G.2
IN1 = (1400, 1600)


def _hits(gold, found, flags=0):
    return [r[0] for r in M.pair_recall(gold, found, flags, CAP)]


def overlap_edges():
    """0 and 1 base of overlap at both ends of either side, in either orientation."""
    specs = []
    for lo, hi in ((900, 1000), (900, 1001), (2000, 2100), (1999, 2100)):  # on side 1: touch left, 1 left, touch right, 1 right
        specs.append((G, [(0, lo, hi, 1) + IN2 + (0,)]))
        specs.append((G, [(1,) + IN2 + (0, lo, hi, 0)]))  # crosswise
    for lo, hi in ((4900, 5000), (4900, 5001), (6000, 6100), (5999, 6100)):  # on side 2
        specs.append((G, [(0,) + IN1 + (1, lo, hi, 0)]))
        specs.append((G, [(1, lo, hi, 0) + IN1 + (0,)]))
    gold, found = units(specs)
    assert _hits(gold, found) == [0, 0, 1, 1, 0, 0, 1, 1] * 2
    rec = M.pair_recall(gold, found, 0, CAP)
    assert [r[1] for r in rec[:8]] == [0, 0, 1, 1, 0, 0, 1, 1] and [r[2] for r in rec[8:]] == [0, 0, 1, 1, 0, 0, 1, 1]
    return gold, found, 0


def orientations():
    """direct only, crosswise only, both ways (one hit, two intervals a side), neither."""
    both_g = (0, 1000, 2000, 0, 1500, 2500, 0)
    specs = [(G, [(0,) + IN1 + (1,) + IN2 + (0,)]),
             (G, [(1,) + IN2 + (0,) + IN1 + (0,)]),
             (both_g, [(0, 1200, 1800, 0, 1600, 1900, 0)]),
             (G, [(0,) + IN1 + (0, 5400, 5600, 0)])]
    gold, found = units(specs)
    rec = M.pair_recall(gold, found, 0, CAP)
    assert [r[0] for r in rec] == [1, 1, 1, 0]
    assert rec[2][1:3] == (700, 400)  # [1200, 1900) of side 1, [1500, 1900) of side 2: both orientations painted
    assert M.listed(gold[2], found) == 2
    return gold, found, 0


def strands(flags):
    """A strand mismatch on one end (either end, either orientation); equal reverse strands meet."""
    specs = [(G, [(0,) + IN1 + (1,) + IN2 + (1,)]),
             (G, [(0,) + IN1 + (1,) + IN2 + (2,)]),
             (G, [(1,) + IN2 + (0,) + IN1 + (1,)]),
             ((0, 1000, 2000, 1, 5000, 6000, 2), [(0,) + IN1 + (1,) + IN2 + (2,)]),
             ((0, 1000, 2000, 1, 5000, 6000, 2), [(1,) + IN2 + (0,) + IN1 + (1,)]),
             ((0, 1000, 2000, 1, 5000, 6000, 3), [(0,) + IN1 + (1,) + IN2 + (0,)])]
    gold, found = units(specs)
    assert _hits(gold, found, flags) == ([1] * 6 if flags else [0, 0, 0, 1, 1, 0])
    return gold, found, flags


def other_chromosome():
    """the same coordinates on another chromosome, on either end."""
    specs = [(G, [(2,) + IN1 + (1,) + IN2 + (0,)]), (G, [(0,) + IN1 + (2,) + IN2 + (0,)]), (G, [(0,) + IN1 + (1,) + IN2 + (0,)])]
    gold, found = units(specs)
    assert _hits(gold, found) == [0, 0, 1]
    return gold, found, 0


def unions():
    """nested, identical and abutting hitting records: the union is not a sum; a hit beyond the gold side on both ends is clipped."""
    def f(a, b, c, d):
        return (0, a, b, 1, c, d, 0)
    specs = [(G, [f(1100, 1900, 5100, 5900), f(1300, 1500, 5300, 5500)]),                 # nested
             (G, [f(1100, 1400, 5100, 5400), f(1100, 1400, 5100, 5400)]),                 # identical
             (G, [f(1100, 1400, 5100, 5400), f(1400, 1700, 5400, 5700)]),                 # abutting
             (G, [f(1100, 1400, 5600, 5900), f(1300, 1800, 5100, 5200)]),                 # overlapping on one side, apart on the other
             (G, [f(500, 2500, 4000, 7000)]),                                             # beyond both ends of both sides
             (G, [f(500, 1100, 5900, 7000), f(1900, 2500, 4000, 5100)])]                  # beyond one end each
    gold, found = units(specs)
    rec = M.pair_recall(gold, found, 0, CAP)
    assert [r[:3] for r in rec] == [(2, 800, 800), (2, 300, 300), (2, 600, 600), (2, 700, 400), (1, 1000, 1000), (2, 200, 200)]
    return gold, found, 0


def _many(n, step=7):
    """n direct hits of G that overlap their neighbours"""
    return [(0, 1000 + step * i % 900, 1000 + step * i % 900 + 50, 1, 5000 + step * i % 900, 5000 + step * i % 900 + 30, 0) for i in range(n)]


def hit_counts():
    """0, 1, WALK - 1, WALK and WALK + 1 hits: the seam of the walk's rounds and of the union's."""
    ns = [0, 1, WALK - 1, WALK, WALK + 1, 2 * WALK, 2 * WALK + 1]
    gold, found = units([(G, _many(n)) for n in ns])
    assert _hits(gold, found) == ns
    return gold, found, 0


def around_the_cap():
    """CAP - 1, CAP and CAP + 1 list entries, by direct hits alone and by records that hit both ways (two entries each)."""
    both_g = (0, 1000, 2000, 0, 1500, 2500, 0)
    both = (0, 1200, 1800, 0, 1600, 1900, 0)
    specs = [(G, _many(CAP - 1)), (G, _many(CAP)), (G, _many(CAP + 1)), (both_g, [both] * (CAP // 2)),
             (both_g, [both] * (CAP // 2) + [(0, 1100, 1150, 0, 2400, 2450, 0)])]
    gold, found = units(specs)
    rec = M.pair_recall(gold, found, 0, CAP)
    assert [M.listed(g, found) for g in gold] == [CAP - 1, CAP, CAP + 1, CAP, CAP + 1]
    assert [r[3] for r in rec] == [0, 0, M.WIDE, 0, M.WIDE] and [r[0] for r in rec] == [CAP - 1, CAP, CAP + 1, CAP // 2, CAP // 2 + 1]
    return gold, found, 0


def sort_window_seams():
    """found ends that start exactly on the two seams of the sort window; one end that spans a whole chromosome's worth of other
    entries counts once; the longest found record next to the shortest."""
    L = 1 << 20  # the longest found end of this call
    g = (0, 3 * L, 3 * L + 1000, 1, 5000, 6000, 0)
    s, e = g[1], g[2]
    found = [(0, s - L + 1, s + 1, 1) + IN2 + (0,),   # starts on the window's first key: one base of overlap
             (0, s - L, s, 1) + IN2 + (0,),           # one below it: touches
             (0, e - 1, e, 1) + IN2 + (0,),           # the window's last key, and the shortest record there is
             (0, e, e + 1, 1) + IN2 + (0,),           # the first key behind it
             (1,) + IN2 + (0, s - L + 1, s + 1, 0),   # the same four as second ends
             (1,) + IN2 + (0, s - L, s, 0), (1,) + IN2 + (0, e - 1, e, 0), (1,) + IN2 + (0, e, e + 1, 0)]
    # a thousand one-base records inside the long ends' span that meet nothing of g: the window holds them all
    found += [(0, s - L + 5 + 900 * i, s - L + 6 + 900 * i, 2, 10 + i, 11 + i, 0) for i in range(1000)]
    gold = [g, (2, 0, 2000, 0, s - L, s + 1, 0)]  # the second is hit crosswise by the thousand, and by nothing else
    rec = M.pair_recall(gold, found, 0, CAP)
    assert rec[0] == (4, 2, 200, 0)
    assert max(f[2] - f[1] for f in found) == L and min(f[2] - f[1] for f in found) == 1
    assert rec[1][0] == 1000 and rec[1][1] == 1000 and rec[1][2] == 1000
    return gold, found, 0


def empties():
    """a gold record with an empty side, a found record with one; both answer nothing."""
    gold = [(0, 1000, 1000, 1, 5000, 6000, 0), (0, 1000, 2000, 1, 5500, 5500, 0), G]
    found = [(0, 900, 2100, 1, 4900, 6100, 0), (0, 1500, 1500, 1, 5000, 6000, 0), (0, 1000, 2000, 1, 5500, 5500, 0)]
    assert M.pair_recall(gold, found, 0, CAP) == [(0, 0, 0, 0), (0, 0, 0, 0), (1, 1000, 1000, 0)]
    return gold, found, 0


def random_draw(rng):
    """at most 300 gold against at most 2,000 found records around a few centres, so that some gold records collect hundreds"""
    ng, nf = int(rng.integers(1, 301)), int(rng.integers(0, 2001))
    fam_chr, fam_at = rng.integers(0, 3, (4, 2)), rng.integers(0, 200000, (4, 2))  # four pairs of places; a record lies at one

    def recs(n, longest):
        fam, swap = rng.integers(0, 4, n), rng.random(n) < 0.3
        c, at = fam_chr[fam], fam_at[fam] + rng.integers(-1500, 1500, (n, 2))
        c, at = np.where(swap[:, None], c[:, ::-1], c), np.maximum(np.where(swap[:, None], at[:, ::-1], at), 0)
        ln = rng.integers(0, longest, (n, 2)) * (rng.random((n, 2)) > 0.02)
        fl = rng.integers(0, 4, n) * (rng.random(n) < 0.3)
        return [(int(c[i, 0]), int(at[i, 0]), int(at[i, 0] + ln[i, 0]), int(c[i, 1]), int(at[i, 1]), int(at[i, 1] + ln[i, 1]), int(fl[i]))
                for i in range(n)]
    return recs(ng, 4000), recs(nf, int(rng.choice([40, 600, 3000]))), int(rng.integers(0, 2))


@functools.lru_cache(maxsize=None)
def tables():
    t = {"overlap_edges": overlap_edges(), "orientations": orientations(), "strands": strands(0), "strands_ignored": strands(M.IGNORE_STRAND),
         "other_chromosome": other_chromosome(), "unions": unions(), "hit_counts": hit_counts(), "around_the_cap": around_the_cap(),
         "sort_window_seams": sort_window_seams(), "empties": empties(),
         "no_gold": ([], [G], 0), "no_found": ([G, (0, 5, 5, 1, 7, 9, 3)], [], 0)}
    rng = np.random.default_rng(2024)
    most = 0
    for d in range(200):
        t["random_%03d" % d] = random_draw(rng)
    for d in range(0, 200, 40):  # (the draws are there for volume; that some gold records collect hundreds is checked on a few)
        g, f, fl = t["random_%03d" % d]
        most = max([most] + [r[0] for r in M.pair_recall(g, f, fl, CAP)])
    assert most >= 100, most
    return t


@functools.lru_cache(maxsize=None)
def expected(name):
    """the model's answer to a table, computed once for every test that asks"""
    gold, found, flags = tables()[name]
    return M.pair_recall(gold, found, flags, CAP)
