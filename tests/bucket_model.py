"""`align bucket` on records as include/sedef_hip.h states it (sdf_bucket_merge), twice.

literal(...)  the reference's sweep word for word (sedef_amd/csrc/host/bucket.cc: merge_hits): the sorted hits one after the
              other, the run's windows as a sorted list of (ref_end, insertion number), lower_bound, the grow loop, `last`; the
              deal with its per-class counters.
closed(...)   what the device forms compute (sedef_amd/csrc/bucket_merge.hip): runs from a prefix maximum of the ORIGINAL query
              ends per segment, every hit's absorption as a fixed point over the run's live slots visited in an ARBITRARY order,
              the survivors by a stable sort on (run, ref_end), the bucket as the place in a stable sort by class, modulo nbins.

A record is a tuple (q_chr, q_start, q_end, r_chr, r_start, r_end, rc); a result record has the bucket behind it.  The cases
the CPU and the GPU tests share are made here (cases())."""
import bisect
import math

import numpy as np

def pair_order(n_groups):
    names = sorted(("tmp_%d_%d.tmp" % (a, b), a * n_groups + b) for a in range(n_groups) for b in range(n_groups))
    out = [0] * (n_groups * n_groups)
    for rank, (_, at) in enumerate(names):
        out[at] = rank
    return out


def prepare(h, chr_group, order, n_groups, extend_ratio, max_extend):
    """Hit::extend, order_sides, the self flag -> (pair, rc, q_chr, r_chr, q_start, r_start, q_end, r_end, self)."""
    qc, qs, qe, rc_, rs, re_, rc = (int(x) for x in h)
    w = max(qe - qs, re_ - rs)
    w = min(max_extend, int(extend_ratio * w))
    qs, qe, rs, re_ = max(0, qs - w), qe + w, max(0, rs - w), re_ + w
    if (qc, qs, qe) > (rc_, rs, re_):
        qc, qs, qe, rc_, rs, re_ = rc_, rs, re_, qc, qs, qe
    pair = order[chr_group[qc] * n_groups + chr_group[rc_]]
    return (pair, rc & 1, qc, rc_, qs, rs, qe, re_, qc == rc_ and qs == rs and qe == re_ and not rc & 1)


def apart(w, h, md):  # boxes [q_start, q_end, r_start, r_end]
    return w[1] + md < h[0] or w[3] < h[2] - md or w[2] > h[3] + md


def cls_of(b):
    return int(math.sqrt(float(b[1] - b[0]) * float(b[3] - b[2]))) // 1000


def sweep_literal(recs, md):
    """recs in sorted order -> merged [(segment key, box)] in the order merge_hits returns."""
    merged, windows, serial = [], [], 0  # windows: sorted [(ref_end, insertion number, box, key)]
    last_key, last_q_end = None, 0
    for r in recs:
        if r[8]:
            continue
        key, h = r[:4], [r[4], r[6], r[5], r[7]]
        new_run = last_key is None or last_q_end + md < h[0] or last_key != key
        if new_run:
            merged += [(w[3], w[2]) for w in windows]
            windows = []
        else:
            grew = True
            while grew:
                grew = False
                k = bisect.bisect_left(windows, (h[2] - md, -1))
                while k < len(windows):
                    w = windows[k][2]
                    if apart(w, h, md):
                        k += 1
                        continue
                    h = [min(h[0], w[0]), max(h[1], w[1]), min(h[2], w[2]), max(h[3], w[3])]
                    del windows[k]
                    grew = True
        bisect.insort(windows, (h[3], serial, h, key))
        serial += 1
        last_q_end = h[1] if new_run else max(h[1], last_q_end)
        last_key = key
    return merged + [(w[3], w[2]) for w in windows]


def sweep_closed(recs, md, rng):
    n = len(recs)
    run_of, runs, prefix = [-1] * n, 0, None
    for i, r in enumerate(recs):  # the segmented prefix maximum
        if i == 0 or recs[i - 1][:4] != r[:4]:
            prefix = None
        if r[8]:
            continue
        if prefix is None or prefix + md < r[4]:
            runs += 1
        run_of[i] = runs - 1
        prefix = r[6] if prefix is None else max(prefix, r[6])
    box = [[r[4], r[6], r[5], r[7]] for r in recs]
    live = [not r[8] for r in recs]
    start = {}
    for i in range(n):
        if run_of[i] >= 0:
            start.setdefault(run_of[i], i)
    for i in range(n):
        if run_of[i] < 0:
            continue
        h = box[i]
        grew = True
        while grew:  # the least fixed point, the slots in any order
            grew = False
            slots = list(range(start[run_of[i]], i))
            rng.shuffle(slots)
            for j in slots:
                if live[j] and not apart(box[j], h, md):
                    w = box[j]
                    h = [min(h[0], w[0]), max(h[1], w[1]), min(h[2], w[2]), max(h[3], w[3])]
                    live[j] = False
                    grew = True
        box[i] = h
    keep = sorted((i for i in range(n) if live[i]), key=lambda i: (run_of[i], box[i][3]))  # (stable)
    return [(recs[i][:4], box[i]) for i in keep]


def records(merged, nbins, closed):
    out = [[key[2], b[0], b[1], key[3], b[2], b[3], key[1], 0] for key, b in merged]
    if closed:
        for p, j in enumerate(sorted(range(len(out)), key=lambda j: cls_of(merged[j][1]))):
            out[j][7] = p % nbins
        return [tuple(r) for r in out]
    top = max([cls_of(b) for _, b in merged] + [0])
    per_class = [0] * (top + 1)
    for _, b in merged:
        per_class[cls_of(b)] += 1
    nxt = [0] * (top + 1)
    for c in range(1, top + 1):
        nxt[c] = (nxt[c - 1] + per_class[c - 1]) % nbins
    for r, (_, b) in zip(out, merged):
        r[7] = nxt[cls_of(b)]
        nxt[cls_of(b)] = (nxt[cls_of(b)] + 1) % nbins
    return [tuple(r) for r in out]


def literal(hits, chr_group, order, n_groups, nbins, extend_ratio=5.0, max_extend=15000, merge_dist=250, **_):
    recs = sorted((prepare(h, chr_group, order, n_groups, extend_ratio, max_extend) for h in hits), key=lambda r: r[:6])
    return records(sweep_literal(recs, merge_dist), nbins, False)


def closed(hits, chr_group, order, n_groups, nbins, extend_ratio=5.0, max_extend=15000, merge_dist=250, seed=0, **_):
    recs = sorted((prepare(h, chr_group, order, n_groups, extend_ratio, max_extend) for h in hits), key=lambda r: r[:6])
    return records(sweep_closed(recs, merge_dist, np.random.default_rng(seed)), nbins, True)


# ---------------------------------------------------------------- the shared cases
def case(hits, nbins=3, n_chr=None, chr_group=None, n_groups=1, **params):
    hits = [tuple(int(x) for x in h) for h in hits]
    if n_chr is None:
        n_chr = max([max(h[0], h[3]) for h in hits] + [0]) + 1
    p = dict(extend_ratio=0.0, max_extend=15000, merge_dist=250)
    p.update(params)
    return dict(hits=hits, chr_group=list(chr_group) if chr_group is not None else [0] * n_chr, order=pair_order(n_groups),
                n_groups=n_groups, nbins=nbins, **p)


def run_of(m, q0=1000, r0=50000, step=100, length=400, chrs=(0, 1), rc=0):
    """m hits of one run that do NOT touch in the reference (each 10,000 further): every one survives, the sweep tests them all."""
    return [(chrs[0], q0 + step * i, q0 + step * i + length, chrs[1], r0 + 10000 * i, r0 + 10000 * i + length, rc) for i in range(m)]


def chained_run(m, q0=1000, r0=50000, step=100, length=400, chrs=(0, 1)):
    """m hits of one run, each touching the one before in both sequences: every hit swallows its predecessor."""
    return [(chrs[0], q0 + step * i, q0 + step * i + length, chrs[1], r0 + step * i, r0 + step * i + length, 0) for i in range(m)]


def staircase(depth=5, gap=70):
    """The new hit touches only window W0; absorbing W0 reaches W1, and so on, `depth` deep.  W(k + 1) ends within merge_dist
    below W(k)'s query start and more than merge_dist below W(k - 1)'s, so the hit's query start has to come down a step at a
    time; in the reference the windows lie in a zigzag around the hit, each within merge_dist of the hull of those before it
    and apart from its neighbours in the query, so that no two of them merge when they arrive.  `gap` fillers, far away in
    the reference, lie between two windows in the sort: the windows sit in different 64-slot steps, the deepest first, and one
    pass over the slots in order finds one of them."""
    hits, far = [], 10 ** 6
    for k in reversed(range(depth)):
        qs = 5000 - 300 * k
        rs = 50300 + 300 * (k // 2) if k % 2 == 0 else 49700 - 300 * (k // 2)
        hits.append((0, qs, qs + 250, 1, rs, rs + 100, 0))
        for i in range(gap):
            hits.append((0, qs + 1 + 4 * i, qs + 51 + 4 * i, 1, far, far + 100, 0))
            far += 5000
    hits.append((0, 5450, 5550, 1, 50000, 50100, 0))
    return hits


def random_hits(rng, n, n_chr=6, span=400000):
    """hostgen.merge_case's draws (starts, lengths 100 .. 1500, a third reversed, a fifth exact duplicates) widened to n_chr
    chromosomes and to coordinates that leave both long runs and lone hits."""
    hits = []
    for _ in range(n):
        if hits and rng.random() < 0.2:
            hits.append(hits[-1])
            continue
        qs, rs = int(rng.integers(0, span)), int(rng.integers(0, span))
        hits.append((int(rng.integers(0, n_chr)), qs, qs + int(rng.integers(100, 1500)), int(rng.integers(0, n_chr)), rs,
                     rs + int(rng.integers(100, 1500)), int(rng.random() < 0.3)))
    return hits


def cases():
    """name -> case; every edge the issue of the device forms lists, small enough for both models."""
    out = {}
    for m in (1, 2, 63, 64, 65, 128, 129, 300):
        out["run_%d" % m] = case(run_of(m) + [(0, 900000, 900400, 1, 5, 405, 0)])
        out["chain_%d" % m] = case(chained_run(m))
    out["staircase"] = case(staircase())
    # a hit whose grown ref_start brings in a window below its first lower_bound: W0 ends at 10400, below the hit's first cut
    # (10900 - 250), and lies too far down in the query; the hit swallows W1 (reference start 10600: the cut comes down to 10350)
    # and X (query start 1000: W0 is no longer apart in the query), and the next pass finds W0
    out["below_lower_bound"] = case([(0, 1000, 3000, 1, 11200, 11300, 0), (0, 1001, 1100, 1, 10000, 10400, 0), (0, 1500, 1600, 1, 10600, 10700, 0),
                                     (0, 1600, 1700, 1, 10900, 11000, 0), (0, 1650, 1700, 1, 90000, 90100, 0)])
    # equal ref_end among the survivors of one run: the flush keeps insertion order
    out["equal_ref_end"] = case([(0, 1000, 1300, 1, 10000, 20000, 0), (0, 1010, 1300, 1, 15000, 20000, 0), (0, 1020, 1300, 1, 19000, 20000, 1),
                                 (0, 1030, 1300, 1, 30000, 40000, 0), (0, 1040, 1300, 1, 35000, 40000, 0)], merge_dist=0)
    self_hit = (0, 1000, 1400, 0, 1000, 1400, 0)
    out["self_first"] = case([self_hit, (0, 1100, 1500, 0, 5000, 5400, 0), (0, 1200, 1600, 0, 5100, 5500, 0)])
    out["self_inside"] = case([(0, 900, 1300, 0, 5000, 5400, 0), self_hit, (0, 1100, 1500, 0, 5100, 5500, 0), (0, 1000, 1400, 0, 1000, 1400, 1)])
    out["self_alone"] = case([self_hit, (1, 1000, 1400, 2, 1000, 1400, 0)], chr_group=[0, 1, 1], n_groups=2)
    # two groups whose adjacent hits would merge by coordinates alone
    out["two_groups"] = case([(0, 1000, 1400, 1, 5000, 5400, 0), (0, 1100, 1500, 2, 5100, 5500, 0), (0, 1150, 1550, 1, 5150, 5550, 0),
                              (0, 1160, 1560, 2, 5160, 5560, 0)], chr_group=[0, 0, 1], n_groups=2)
    # equal names on both sides, ordered by start and then by end
    out["same_names"] = case([(0, 5000, 5400, 0, 1000, 1400, 0), (0, 1000, 1500, 0, 1000, 1400, 0), (0, 1000, 1400, 0, 1000, 1500, 1),
                              (0, 5100, 5500, 0, 1100, 1500, 0)])
    for md in (0, 250):
        out["merge_dist_%d" % md] = case([(0, 1000, 1400, 1, 5000, 5400, 0), (0, 1400, 1800, 1, 5400, 5800, 0), (0, 1801, 2200, 1, 5801, 6200, 0),
                                          (0, 2450, 2800, 1, 6450, 6800, 0), (0, 3051, 3400, 1, 7051, 7400, 0)], merge_dist=md)
    # extension clamped at 0 and at max_extend, on either side
    out["extend"] = case([(0, 100, 400, 1, 50000, 50200, 0), (0, 90000, 99000, 1, 300, 9300, 1), (2, 10, 20, 0, 10, 30, 0), (1, 0, 0, 1, 0, 0, 1)],
                         extend_ratio=5.0, max_extend=15000)
    out["both_strands"] = case([(0, 1000 + 10 * i, 1400 + 10 * i, 1, 5000 + 10 * i, 5400 + 10 * i, i & 1) for i in range(20)])
    # class products k^2 and k^2 - 1, and products beyond 2^53
    cls = []
    for k in (1000, 2000, 46341000):
        for qlen, rlen in ((k, k), (k - 1, k + 1)):  # (k - 1)(k + 1) = k^2 - 1
            at = len(cls) * 3
            cls.append((at, 0, qlen, at + 1, 0, rlen, 0))
    cls.append((30, 0, 94906267, 31, 0, 94906267, 0))      # 94906267^2 = 2^53 + 2.5e8: the product rounds
    cls.append((32, 0, 2147483647, 33, 0, 2147483647, 0))  # (2^31 - 1)^2
    cls.append((34, 0, 134217729, 35, 0, 67108865, 0))     # (2^27 + 1)(2^26 + 1) = 2^53 + ... + 1: odd, not representable
    out["classes"] = case(cls, nbins=3, max_extend=0, merge_dist=0)
    for nb in (1, 3, 1000):
        out["nbins_%d" % nb] = case(random_hits(np.random.default_rng(nb), 120, n_chr=3, span=20000), nbins=nb, chr_group=[0, 1, 0], n_groups=2,
                                    extend_ratio=5.0)
    out["empty"] = case([])
    return out
