"""The search driver's two statements in Python, independent of the library's code for them.

initial_search(...)   the reference's initial_search (src/search_main.cc:41-82) as written, window by window: the loop of
                      replay() in tests/test_search_found_cpu.py over the record-list model of the tree (found_model.py) and the
                      host forms of roll / filter / extend / filter -- each pinned on the reference by its own tests -- with the
                      schedule computed literally (next_to_attain from the reported hits' lengths), completed-WIDE hits counted
                      as hits, parse_hits (src/search.cc) and the three counters.  The reference's search.cc needs Boost and
                      cannot be built here, so this composition is what sdf_search_pair_host is compared with.
accept(...)           one round of the acceptance step as include/sedef_hip.h states it.

Rounds for the acceptance step are made by Round: windows with hand-written intervals."""
import numpy as np

import found_model as FM
import minim_model as M
import search_model as S

FAIL = 1 | 2 | 8  # FILTER_UPPER_FAIL | FILTER_QGRAM_FAIL | FILTER_SKIPPED
EXT_SKIPPED, EXT_WIDE, EXT_NOLIMIT = 1, 2, 4
ROLL_WIDE, ROLL_BADWINDOW = 1, 2
WIN_WIDE, WIN_FOUND_WIDE = 4, 8
MAX_KEPT = 512
INCOMPLETE, OVERFLOW = 1, 2
MAX_ERROR = 0.30


def parse_hits(hits):
    """src/search.cc parse_hits on (query_start, query_end, ref_start, ref_end, ...) tuples: the survivors, in order."""
    keep = []
    for h, a in enumerate(hits):
        dropped = any(p != h and a[2] >= b[2] and a[3] <= b[3] and a[0] >= b[0] and a[1] <= b[1] for p, b in enumerate(hits))
        if not dropped:
            keep.append(a)
    return keep


def greedy_schedule(q, min_read_size, uppercase_seeds, max_error=MAX_ERROR):
    """Fact 1: the windows that run, from q's loc and status alone."""
    out, nxt = [], 0
    for i in range(len(q)):
        loc = int(q["loc"][i])
        if loc < nxt or (uppercase_seeds and q["status"][i] != 0):
            continue
        out.append(i)
        nxt = int(loc + (min_read_size * max_error) / 2)
    return out


def inputs(seed, same_genome, init_len, r_rc=False):
    """A drawn pair as replay() draws it; with r_rc the reference is searched reverse-complemented."""
    from test_search_found_cpu import draw_sequence
    rng = np.random.default_rng(seed)
    unit = rng.integers(0, 4, int(rng.integers(180, 260)))
    qs = draw_sequence(rng, unit, 6, 1000)
    rs = qs if same_genome else draw_sequence(rng, unit, 7, 900)
    if r_rc:  # the pool holds the other strand, so that the searched one carries the repeats
        rs = M.rev_comp(rs)
    assert 3000 <= len(qs) <= 6000 and 3000 <= len(rs) <= 6000
    pool = qs if same_genome else qs + rs
    return dict(pool=pool, q_range=(0, len(qs), 0), r_range=(0, len(qs), 0) if same_genome else (len(qs), len(rs), 1 if r_rc else 0),
                same_genome=same_genome, init_len=init_len, k=8, w=4, limit=[max(1, s // 8) for s in range(200)])


def initial_search(extz2, I):
    """initial_search on the inputs I.  Returns the reported hits as SEARCH_PAIR_HIT rows, the counters, the windows that ran,
    and what the run showed (for the tests' own asserts)."""
    pool, init_len, same_genome, limit = I["pool"], I["init_len"], I["same_genome"], I["limit"]
    q_off, len_q, _ = I["q_range"]
    r_off, len_r, r_rc = I["r_range"]
    qs = pool[q_off:q_off + len_q]
    rs = pool[r_off:r_off + len_r]
    if r_rc:
        rs = M.rev_comp(rs)
    q = S.records(M.get_minimizers(qs, I["k"], I["w"], True))
    r = q if same_genome else S.records(M.get_minimizers(rs, I["k"], I["w"], True))
    r_sorted = S.index_order(r)
    threshold = M.index([(int(h), int(loc), int(st)) for h, loc, st in zip(r["hash"], r["loc"], r["status"])])[1]
    kw = dict(r_threshold=threshold, len_q=len_q, init_len=init_len, same_genome=same_genome, uppercase_seeds=1, limit=limit)
    fparams = extz2.filter_params()
    eparams = extz2.extend_params(same_genome=bool(same_genome), max_sd_size=int(2.5 * init_len))
    min_read_size = init_len
    walk = FM.Walker(q, r_sorted, **kw)
    nq = len(q)
    found, reported, ran = [], [], []
    count = dict(attempted=0, jaccard_failed=0, interval_failed=0)
    seen = dict(failed_in_window=0, failed_by_earlier=0, lost=0, dropped=0)
    next_to_attain = 0
    for i in range(nq):
        loc = int(q["loc"][i])
        if loc < next_to_attain:
            continue
        if q["status"][i] != 0:  # DoUppercaseSeeds
            continue
        ran.append(i)
        nf0 = len(found)
        qsz, nm, ng, c, flags, T = walk.window(i, FM.RecordList(found, nf0).excluded)
        seen["lost"] += len(T) < len(walk.window(i, lambda a, b: False)[5])
        hits = []
        if T:
            T_arr = np.array(T, np.int64).astype("<i4").view(S.INTERVAL).reshape(-1)
            w1 = np.zeros(nq, S.WINDOW)
            w1[i] = (qsz, nm, ng, len(c), flags)
            f1 = np.array([0] * (i + 1) + [len(T)] * (nq - i), np.uint64)
            code, rolls = extz2.search_roll_host(q, w1, f1, T_arr, r, len_r, init_len, limit)
            assert code == 0
            code, tasks = extz2.search_filter_tasks_host(q, w1, f1, T_arr, rolls, len_q, len_r, init_len, q_off, 0, r_off, r_rc, 1)
            assert code == 0
            code, frec = extz2.search_filter_host(pool, tasks, fparams)
            assert code == 0
            code, ext = extz2.search_extend_host(q, w1, f1, T_arr, rolls, frec, r, len_q, len_r, init_len, limit, eparams)
            assert code == 0
            code, htasks = extz2.search_hit_tasks_host(ext, len_q, len_r, q_off, 0, r_off, r_rc)
            assert code == 0
            code, hrec = extz2.search_filter_host(pool, htasks, fparams)
            assert code == 0
            for t in range(len(T)):
                count["attempted"] += 1
                if rolls["jaccard"][t] < 0:
                    count["jaccard_failed"] += 1
                    continue
                args = (loc, loc + init_len, int(rolls["ref_start"][t]), int(rolls["ref_end"][t]), min_read_size)
                if FM.RecordList(found, len(found)).is_overlap(*args):
                    count["interval_failed"] += 1
                    by_earlier = FM.RecordList(found, nf0).is_overlap(*args)
                    seen["failed_by_earlier"] += by_earlier
                    seen["failed_in_window"] += not by_earlier
                    continue
                if frec["flags"][t] & FAIL or ext["flags"][t] & (EXT_SKIPPED | EXT_NOLIMIT) or hrec["flags"][t] & FAIL:
                    continue
                h = tuple(int(ext[f][t]) for f in ("query_start", "query_end", "ref_start", "ref_end", "jaccard"))
                hits.append(h)
                found.append(h[:4])
        kept = parse_hits(hits)
        seen["dropped"] += len(hits) - len(kept)
        min_len = len_q
        for h in kept:
            min_len = min(min_len, h[1] - h[0])
            reported.append((i,) + h)
        next_to_attain = int(loc + (min_read_size * MAX_ERROR) / 2) if min_len >= min_read_size else loc
    out = np.zeros(len(reported), extz2.SEARCH_PAIR_HIT_DTYPE)
    for k, row in enumerate(reported):
        out[k] = row
    return dict(hits=out, count=count, ran=ran, seen=seen, q=q, found=found, min_read_size=min_read_size)


# ---- the acceptance step ----

class Round:
    """A round by hand: window(loc, intervals, flags, act) in ascending loc; an interval is made by iv()."""

    def __init__(self, init_len=100, min_read_size=100):
        self.init_len, self.min_read_size = init_len, min_read_size
        self.locs, self.flags, self.act, self.ivs = [], [], [], []

    @staticmethod
    def iv(hit=None, ref=(5000, 5100), jaccard=3, verdict=0, f1=0, f2=0, hflags=0, rflags=0, hj=7):
        """hit: (query_start, query_end, ref_start, ref_end), None for a zero record."""
        return dict(hit=hit or (0, 0, 0, 0), ref=ref, jaccard=jaccard, verdict=verdict, f1=f1, f2=f2, hflags=hflags, rflags=rflags, hj=hj)

    def window(self, loc, intervals=(), flags=0, act=True):
        assert not self.locs or loc > self.locs[-1]
        if act:
            self.act.append(len(self.locs))
        self.locs.append(loc)
        self.flags.append(flags)
        self.ivs.append(list(intervals))
        return self

    def arrays(self, extz2):
        nq = len(self.locs)
        q = S.records([(1 + i, loc, 0) for i, loc in enumerate(self.locs)])
        windows = np.zeros(nq, S.WINDOW)
        windows["flags"] = self.flags
        windows["query_size"], windows["n_members"] = 1, 1
        first = np.zeros(nq + 1, np.uint64)
        flat = [v for ivs in self.ivs for v in ivs]
        first[1:] = np.cumsum([len(ivs) for ivs in self.ivs])
        n = len(flat)
        rolls, hits = np.zeros(n, extz2.SEARCH_ROLL_DTYPE), np.zeros(n, extz2.SEARCH_HIT_DTYPE)
        overlap, filt, hfilt = np.zeros(n, np.uint32), np.zeros(n, extz2.FILTER_REC_DTYPE), np.zeros(n, extz2.FILTER_REC_DTYPE)
        for t, v in enumerate(flat):
            rolls[t] = (v["ref"][0], v["ref"][1], 0, 0, v["jaccard"], v["rflags"])
            hits[t] = v["hit"] + (v["hj"], 0, 0, 0, 0, v["hflags"])
            overlap[t], filt["flags"][t], hfilt["flags"][t] = v["verdict"], v["f1"], v["f2"]
        return dict(q=q, act=np.array(self.act, np.uint32), windows=windows, first=first, rolls=rolls, overlap=overlap, filt=filt,
                    hits=hits, hit_filter=hfilt, init_len=self.init_len, min_read_size=self.min_read_size)


def accept(A, found, out, found_cap, out_cap, window_base=0, n_max=None):
    """One round (the arrays of Round.arrays) against the lists found / out (rows).  Returns (status dict, found rows, out rows)."""
    q, first, rolls, hits = A["q"], A["first"], A["rolls"], A["hits"]
    init_len, mrs = A["init_len"], A["min_read_size"]
    n_max = len(rolls) if n_max is None else n_max
    per_window = []
    for i in (int(x) for x in A["act"]):
        loc = int(q["loc"][i])
        t0, t1 = int(first[i]), int(first[i + 1])
        incomplete = bool(A["windows"]["flags"][i] & (WIN_WIDE | WIN_FOUND_WIDE)) or t1 > n_max
        kept, c = [], [0, 0, 0]
        for t in (range(t0, t1) if t1 <= n_max else ()):
            R, H = rolls[t], hits[t]
            incomplete |= bool(R["flags"] & ROLL_WIDE and R["ref_end"] == 0) or bool(R["flags"] & ROLL_BADWINDOW)
            incomplete |= bool(H["flags"] & EXT_WIDE and H["query_end"] == 0)
            c[0] += 1
            if R["jaccard"] < 0:
                c[1] += 1
            elif A["overlap"][t]:
                c[2] += 1
            elif FM.RecordList([k[:4] for k in kept[:MAX_KEPT]], MAX_KEPT).is_overlap(loc, loc + init_len, int(R["ref_start"]),
                                                                                         int(R["ref_end"]), mrs):
                c[2] += 1
            elif not (A["filt"]["flags"][t] & FAIL or H["flags"] & (EXT_SKIPPED | EXT_NOLIMIT) or A["hit_filter"]["flags"][t] & FAIL):
                kept.append(tuple(int(H[f]) for f in ("query_start", "query_end", "ref_start", "ref_end", "jaccard")))
        incomplete |= len(kept) > MAX_KEPT
        per_window.append((i, loc, incomplete, kept, c))
    frontier, reach = len(per_window), 0
    for j, (i, loc, incomplete, kept, c) in enumerate(per_window):
        if reach > loc or incomplete:
            frontier = j
            break
        reach = max([reach] + [k[1] for k in kept])
    new_found, new_out, total = list(found), list(out), [0, 0, 0]
    for i, loc, incomplete, kept, c in per_window[:frontier]:
        new_found += [k[:4] for k in kept]
        new_out += [(window_base + i,) + k for k in parse_hits(kept)]
        total = [a + b for a, b in zip(total, c)]
    over = len(new_found) > found_cap or len(new_out) > out_cap
    status = dict(frontier=0 if over else frontier,
                  flags=OVERFLOW if over else INCOMPLETE if frontier < len(per_window) and per_window[frontier][2] else 0,
                  nf=len(found) if over else len(new_found), n_out=len(out) if over else len(new_out), need_found=len(new_found),
                  need_out=len(new_out), attempted=0 if over else total[0], jaccard_failed=0 if over else total[1],
                  interval_failed=0 if over else total[2])
    return status, (list(found) if over else new_found), (list(out) if over else new_out)
