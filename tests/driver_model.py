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
# the driver's own sizes: SDF_PAIR_* of include/sedef_hip.h as extz2 mirrors them
from sedef_amd.extz2 import PAIR_ENTRIES_START, PAIR_INTERVALS_START, PAIR_LONG_BATCH, PAIR_LONG_MAX, PAIR_ROUND_WINDOWS  # noqa: E402,F401


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
    P = Pair(extz2, I)
    q, nq, len_q, min_read_size = P.q, len(P.q), P.len_q, P.min_read_size
    found, reported, ran, nf_before = [], [], [], []
    count = dict(attempted=0, jaccard_failed=0, interval_failed=0)
    seen = dict(failed_in_window=0, failed_by_earlier=0, lost=0, dropped=0, max_meeting=0, max_grow=0)
    next_to_attain = 0
    for i in range(nq):
        loc = int(q["loc"][i])
        if loc < next_to_attain:
            continue
        if P.uppercase_seeds and q["status"][i] != 0:  # DoUppercaseSeeds
            continue
        ran.append(i)
        nf_before.append(len(found))
        seen["max_meeting"] = max(seen["max_meeting"], FM.RecordList(found, len(found)).meeting(loc, P.init_len))
        kept = P.window(i, found, count, seen)
        min_len = len_q
        for h in kept:
            min_len = min(min_len, h[1] - h[0])
            reported.append((i,) + h)
        next_to_attain = int(loc + (min_read_size * P.max_error) / 2) if min_len >= min_read_size else loc
    return dict(hits=hit_rows(extz2, reported), count=count, ran=ran, seen=seen, q=q, found=found, min_read_size=min_read_size,
                nf_before=nf_before)


def hit_rows(extz2, reported):
    out = np.zeros(len(reported), extz2.SEARCH_PAIR_HIT_DTYPE)
    for k, row in enumerate(reported):
        out[k] = row
    return out


def pair_kwargs(extz2, I):
    """The inputs' parameters as search_pair / search_pair_host take them."""
    return dict(k=I["k"], w=I["w"], min_read_size=I["init_len"], same_genome=I["same_genome"], limit=I["limit"],
                separate_lowercase=I.get("separate_lowercase", 1), uppercase_seeds=I.get("uppercase_seeds", 1),
                filter=extz2.filter_params(max_error=I.get("max_error", MAX_ERROR)),
                extend=extz2.extend_params(same_genome=bool(I["same_genome"]), max_sd_size=I.get("max_sd_size", int(2.5 * I["init_len"]))))


class Pair:
    """The arrays and parameters of a pair, prepared once: both sequences as searched (reverse-complemented under the RC flag
    of their range), their minimizers, the reference's index -- and window(), the per-window step of initial_search."""

    def __init__(self, extz2, I):
        self.extz2, self.pool, self.init_len, self.same_genome, self.limit = extz2, I["pool"], I["init_len"], I["same_genome"], I["limit"]
        self.q_off, self.len_q, self.q_rc = I["q_range"]
        self.r_off, self.len_r, self.r_rc = I["r_range"]
        self.uppercase_seeds, sep = I.get("uppercase_seeds", 1), I.get("separate_lowercase", 1)
        self.max_error = I.get("max_error", MAX_ERROR)
        qs = self.pool[self.q_off:self.q_off + self.len_q]
        rs = self.pool[self.r_off:self.r_off + self.len_r]
        if self.q_rc:
            qs = M.rev_comp(qs)
        if self.r_rc:
            rs = M.rev_comp(rs)
        self.q = S.records(M.get_minimizers(qs, I["k"], I["w"], bool(sep)))
        self.r = self.q if self.same_genome else S.records(M.get_minimizers(rs, I["k"], I["w"], bool(sep)))
        self.r_sorted = S.index_order(self.r)
        self.threshold = M.index([(int(h), int(loc), int(st)) for h, loc, st in zip(self.r["hash"], self.r["loc"], self.r["status"])])[1]
        self.wkw = dict(r_threshold=self.threshold, len_q=self.len_q, init_len=self.init_len, same_genome=self.same_genome,
                        uppercase_seeds=self.uppercase_seeds, limit=self.limit)
        self.fparams = extz2.filter_params(max_error=self.max_error)
        self.eparams = extz2.extend_params(same_genome=bool(self.same_genome), max_sd_size=I.get("max_sd_size", int(2.5 * self.init_len)))
        self.min_read_size = self.init_len
        self.walk = FM.Walker(self.q, self.r_sorted, **self.wkw)

    def stages(self, windows, first, T_arr, verdicts=None):
        """roll / filter / extend / filter by their host forms over the intervals T_arr of `windows`; verdicts: the is_overlap
        answers whose intervals get a skip task, as sdf_search_overlap_device rewrites them."""
        extz2, q, r = self.extz2, self.q, self.r
        tail = (self.q_off, self.q_rc, self.r_off, self.r_rc)
        code, rolls = extz2.search_roll_host(q, windows, first, T_arr, r, self.len_r, self.init_len, self.limit)
        assert code == 0
        code, tasks = extz2.search_filter_tasks_host(q, windows, first, T_arr, rolls, self.len_q, self.len_r, self.init_len, *tail, 1)
        assert code == 0
        if verdicts is not None:
            skip = np.zeros(1, extz2.FILTER_TASK_DTYPE)
            skip["flags"] = extz2.FILTER_SKIP
            tasks[np.flatnonzero(verdicts)] = skip[0]
        code, frec = extz2.search_filter_host(self.pool, tasks, self.fparams)
        assert code == 0
        code, ext = extz2.search_extend_host(q, windows, first, T_arr, rolls, frec, r, self.len_q, self.len_r, self.init_len, self.limit,
                                             self.eparams)
        assert code == 0
        code, htasks = extz2.search_hit_tasks_host(ext, self.len_q, self.len_r, *tail)
        assert code == 0
        code, hrec = extz2.search_filter_host(self.pool, htasks, self.fparams)
        assert code == 0
        return rolls, frec, ext, hrec

    def grow(self, i, H):
        """The records by which the hit H of window i grew q's winnow range: in front of the window's first member, and behind
        its last one."""
        nm = int(np.searchsorted(self.q["loc"], int(self.q["loc"][i]) + self.init_len, "right")) - i
        return max(i - int(H["q_winnow_start"]), int(H["q_winnow_end"]) - (i + nm))

    def window(self, i, found, count, seen=None):
        """Window i against the whole list `found`, which receives its kept hits.  Returns the hits parse_hits leaves."""
        q, nq, init_len, mrs = self.q, len(self.q), self.init_len, self.min_read_size
        loc = int(q["loc"][i])
        # (only a record with q_start <= loc + init_len and q_end > loc can cover a member of the window, or its loc)
        near = [R for R in found if R[0] <= loc + init_len and R[1] > loc]
        nf0 = len(near)
        qsz, nm, ng, c, flags, T = self.walk.window(i, FM.RecordList(near, nf0).excluded)
        if seen is not None:
            seen["lost"] += len(T) < len(self.walk.window(i, lambda a, b: False)[5])
        hits = []
        if T:
            T_arr = np.array(T, np.int64).astype("<i4").view(S.INTERVAL).reshape(-1)
            w1 = np.zeros(nq, S.WINDOW)
            w1[i] = (qsz, nm, ng, len(c), flags)
            f1 = np.array([0] * (i + 1) + [len(T)] * (nq - i), np.uint64)
            rolls, frec, ext, hrec = self.stages(w1, f1, T_arr)
            for t in range(len(T)):
                count["attempted"] += 1
                if rolls["jaccard"][t] < 0:
                    count["jaccard_failed"] += 1
                    continue
                args = (loc, loc + init_len, int(rolls["ref_start"][t]), int(rolls["ref_end"][t]), mrs)
                if FM.RecordList(near, len(near)).is_overlap(*args):
                    count["interval_failed"] += 1
                    if seen is not None:
                        by_earlier = FM.RecordList(near, nf0).is_overlap(*args)
                        seen["failed_by_earlier"] += by_earlier
                        seen["failed_in_window"] += not by_earlier
                    continue
                if frec["flags"][t] & FAIL or ext["flags"][t] & (EXT_SKIPPED | EXT_NOLIMIT) or hrec["flags"][t] & FAIL:
                    continue
                h = tuple(int(ext[f][t]) for f in ("query_start", "query_end", "ref_start", "ref_end", "jaccard"))
                hits.append(h)
                found.append(h[:4])
                near.append(h[:4])
                if seen is not None:
                    seen["max_grow"] = max(seen["max_grow"], self.grow(i, ext[t]))
        kept = parse_hits(hits)
        if seen is not None:
            seen["dropped"] += len(hits) - len(kept)
        return kept


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


# ---- the driver's rounds ----

def rounds(extz2, I, round_windows, debug_host_every=0, capacities=False):
    """sdf_search_pair's loop (include/sedef_hip.h, the search driver's section) from parts that are pinned elsewhere: the
    schedule, per round the windows of the slice against the found list as it stands at the round's start, the stages' host
    forms as initial_search composes them, and accept() for the frontier.  What the device leaves for the host -- a WIDE or
    FOUND_WIDE window, a roll that is WIDE, a long growth beyond the PAIR_LONG_MAX a round finishes -- makes its window
    incomplete, and the frontier window of such a round is completed as initial_search completes it.  Capacities are unlimited;
    with capacities=True they are the driver's: the intervals a round holds (a window whose records lie beyond them is
    incomplete, a round with more is repeated when it accepted nothing and taken as far as it goes otherwise, the capacity
    twice the need either way) and the device list's (2 * want + 1024 when nf + the interval capacity passes it).  `events`
    then lists ("repeat" | "partial", round, intervals, capacity), ("found_grew", nf, want, capacity before) and ("entries",
    round, bin entries, capacity): a round whose found list has more bin entries than the capacity is repeated with twice
    the need.  What such a round counts as its intervals is the device's own, so when it also needed more intervals than the
    capacity `entries_short` is set, and the three stats are then lower bounds.
    Returns dict(hits, count, per_round, rounds, windows_run, windows_host, scheduled); per_round: (first scheduled index, na,
    intervals needed, found entries needed, nf at the start, frontier, flags, long growths) per round; the found list at every
    round's start is in `found_at`."""
    P = Pair(extz2, I)
    q, nq, init_len = P.q, len(P.q), P.init_len
    qloc = q["loc"].astype(np.int64)
    sched = greedy_schedule(q, P.min_read_size, P.uppercase_seeds, P.max_error)
    size = round_windows if round_windows else PAIR_ROUND_WINDOWS
    every = debug_host_every
    found, reported, per_round, found_at = [], [], [], []
    count = dict(attempted=0, jaccard_failed=0, interval_failed=0)
    stat = dict(rounds=0, windows_run=0, windows_host=0)
    cap = dict(iv=PAIR_INTERVALS_START, ent=PAIR_ENTRIES_START, found=0)
    events, entries_short = [], False

    def sync_found(want, nf_now):  # pair_sync_found
        if capacities and want > cap["found"]:
            events.append(("found_grew", nf_now, want, cap["found"]))
            cap["found"] = 2 * want + 1024

    def host_one(i):
        nf0 = len(found)
        for h in P.window(i, found, count):
            reported.append((i,) + h)
        stat["windows_host"] += 1
        stat["windows_run"] += 1
        sync_found(len(found), nf0)

    s0 = 0
    while s0 < len(sched):
        if every and s0 % every == every - 1:
            host_one(sched[s0])
            s0 += 1
            continue
        na = min(size, len(sched) - s0)
        if every:
            na = min(na, every - 1 - s0 % every)
        act = sched[s0:s0 + na]
        i0, e = act[0], act[-1]
        while e < nq and qloc[e] - qloc[act[-1]] <= init_len:
            e += 1
        nf = len(found)
        found_at.append(list(found))
        sync_found(nf + cap["iv"], nf)
        frows = FM.found_records(found)
        # the slice's windows, every one seeing the whole list; the device form leaves a WIDE or FOUND_WIDE window without intervals
        rc, first_s, win_s, T_s, used = extz2.search_windows_found_host(q[i0:e], P.r_sorted, P.threshold, P.len_q, init_len, P.same_genome,
                                                                        P.uppercase_seeds, P.limit, frows, np.full(e - i0, nf, np.uint32))
        assert rc == 0
        first_s = np.asarray(first_s, np.int64)
        per = np.diff(first_s)
        wide = (win_s["flags"] & (WIN_WIDE | WIN_FOUND_WIDE)) != 0
        keep = np.repeat(~wide, per)
        T_arr = np.ascontiguousarray(T_s[:int(first_s[-1])][keep])
        per = np.where(wide, 0, per)
        windows = np.zeros(nq, S.WINDOW)
        windows[i0:e] = win_s
        windows["n_candidates"][i0:e][wide] = 0
        first = np.zeros(nq + 1, np.uint64)
        first[i0 + 1:e + 1] = np.cumsum(per)
        first[e + 1:] = first[e]
        n = int(first[nq])
        n_max = min(n, cap["iv"]) if capacities else n
        n_long = 0
        if n:
            owner = np.repeat(np.arange(nq), np.diff(first.astype(np.int64)))
            rolls = extz2.search_roll_host(q, windows, first, T_arr, P.r, P.len_r, init_len, P.limit)[1]
            rc, verdicts = extz2.search_overlap_host(q, first, rolls, frows, np.full(n, nf, np.uint32), init_len, P.min_read_size)
            assert rc == 0
            rolls, frec, ext, hrec = P.stages(windows, first, T_arr, verdicts)
            # what the device leaves for the host
            left = (rolls["flags"] & (ROLL_WIDE | ROLL_BADWINDOW)) != 0
            long_ = ((ext["flags"] & EXT_WIDE) != 0) & ~left & (np.arange(n) < n_max)
            n_long = int(long_.sum())
            left |= ((ext["flags"] & EXT_WIDE) != 0) & ~long_
            left[np.flatnonzero(long_)[PAIR_LONG_MAX:]] = True
            dev_windows = windows.copy()
            dev_windows["flags"][np.unique(owner[left])] |= WIN_WIDE
        else:
            rolls, ext = np.zeros(0, extz2.SEARCH_ROLL_DTYPE), np.zeros(0, extz2.SEARCH_HIT_DTYPE)
            frec = hrec = np.zeros(0, extz2.FILTER_REC_DTYPE)
            verdicts, dev_windows = np.zeros(0, np.uint32), windows
        A = dict(q=q, act=np.array(act, np.uint32), windows=dev_windows, first=first, rolls=rolls, overlap=verdicts, filt=frec, hits=ext,
                 hit_filter=hrec, init_len=init_len, min_read_size=P.min_read_size)
        status, new_found, out = accept(A, found, [], 1 << 62, 1 << 62, n_max=n_max)
        stat["rounds"] += 1
        stat["windows_run"] += na
        entries = extz2.found_entries(frows)
        per_round.append((s0, na, n, entries, nf, status["frontier"], status["flags"], n_long))
        if capacities:
            if entries > cap["ent"]:  # the index was incomplete: nothing of the round holds, and it is repeated
                events.append(("entries", len(per_round) - 1, entries, cap["ent"]))
                cap["ent"] = 2 * entries
                # (what such a round counts as its intervals is the device's own: only with room to spare is the rest exact)
                entries_short |= n > cap["iv"]
                continue
            if n > cap["iv"]:
                repeat = status["frontier"] == 0
                events.append(("repeat" if repeat else "partial", len(per_round) - 1, n, cap["iv"]))
                cap["iv"] = 2 * n
                if repeat:
                    continue  # the same round again, with room
                status["flags"] &= ~INCOMPLETE  # (incomplete for want of room, not for the host)
        found = new_found
        reported += out
        for f in count:
            count[f] += status[f]
        s0 += status["frontier"]
        if status["flags"] & INCOMPLETE:
            host_one(sched[s0])
            s0 += 1
        else:
            assert status["frontier"] > 0
    return dict(hits=hit_rows(extz2, reported), count=count, per_round=per_round, found_at=found_at, scheduled=len(sched), sched=sched, events=events,
                entries_short=entries_short, **stat)


# ---- inputs that reach the driver's paths (tests/test_search_driver_paths_cpu.py states what each must show) ----

LETTERS = np.frombuffer(b"ACGT", np.uint8)


def tandem(rng, unit, copies, rate):
    """`copies` copies of unit back to back, each with its own substitutions at `rate`."""
    parts = []
    for _ in range(copies):
        u = unit.copy()
        hit = rng.random(len(u)) < rate
        u[hit] = (u[hit] + rng.integers(1, 4, int(hit.sum()))) % 4
        parts.append(u)
    return np.concatenate(parts)


def arrays_input(seed, unit_len, q_copies, r_copies, rate, init_len, flank=150, **more):
    """A query with a tandem array of q_copies diverged copies of a unit between random flanks, and a reference with r_copies."""
    rng = np.random.default_rng(seed)
    unit = rng.integers(0, 4, unit_len)

    def seq(copies):
        return LETTERS[np.concatenate([rng.integers(0, 4, flank), tandem(rng, unit, copies, rate), rng.integers(0, 4, flank)])].tobytes()
    qs, rs = seq(q_copies), seq(r_copies)
    I = dict(pool=qs + rs, q_range=(0, len(qs), 0), r_range=(len(qs), len(rs), 0), same_genome=0, init_len=init_len, k=8, w=4,
             limit=[max(1, s // 8) for s in range(200)])
    I.update(more)
    return I


def placed_input(seed, init_len, q_off=0, q_rc=False, r_rc=False, lower=(), n_run=None, **more):
    """The pair of inputs(seed, 0, init_len) with the query behind q_off other characters of the pool; under q_rc / r_rc the pool
    holds the other strand of that sequence, so that the searched one carries the repeats.  lower: (start, end) stretches of
    the query and of the reference in lowercase; n_run: (start, length) of a run of N in the query."""
    from test_search_found_cpu import draw_sequence
    rng = np.random.default_rng(seed)
    unit = rng.integers(0, 4, int(rng.integers(180, 260)))
    qs = bytearray(draw_sequence(rng, unit, 6, 1000))
    rs = bytearray(draw_sequence(rng, unit, 7, 900))
    for a, b in lower:
        qs[a:b] = bytes(qs[a:b]).lower()
        rs[a + 100:b + 100] = bytes(rs[a + 100:b + 100]).lower()
    if n_run:
        qs[n_run[0]:n_run[0] + n_run[1]] = b"N" * n_run[1]
    qs, rs = bytes(qs), bytes(rs)
    head = LETTERS[rng.integers(0, 4, q_off)].tobytes()
    pool = head + (M.rev_comp(qs) if q_rc else qs) + (M.rev_comp(rs) if r_rc else rs)
    I = dict(pool=pool, q_range=(q_off, len(qs), int(q_rc)), r_range=(q_off + len(qs), len(rs), int(r_rc)), same_genome=0,
             init_len=init_len, k=8, w=4, limit=[max(1, s // 8) for s in range(200)])
    I.update(more)
    return I


H_CASE = dict(lower=((700, 1100), (2300, 2450)), n_run=(1800, 40))


def path_inputs():
    """name -> inputs, one per path of the driver; drawn here, the seeds and sizes chosen on the CPU so that the asserts of
    tests/test_search_driver_paths_cpu.py hold."""
    empty = placed_input(31, 60, lower=((0, 1 << 20),))
    return {
        "b": arrays_input(5, 200, 4, 40, 0.04, 60),
        "e": arrays_input(9, 100, 2, 300, 0.04, 60),
        "g_off": placed_input(17, 60, q_off=517),
        "g_off_rrc": placed_input(19, 75, q_off=1033, r_rc=True),
        "g_qrc": placed_input(23, 60, q_rc=True),
        "g_qrc_rrc": placed_input(37, 75, q_rc=True, r_rc=True),
        "h": placed_input(41, 60, **H_CASE),
        "h_all_seeds": placed_input(41, 60, uppercase_seeds=0, **H_CASE),
        "h_one_case": placed_input(41, 60, separate_lowercase=0, **H_CASE),
        "h_max_error": placed_input(41, 60, max_error=0.2, **H_CASE),
        "f": long_input(3, 8860),
        "f_many": long_input(3, 9100),
        "f_host": copies_input(3, 8900, 18, rate=0.003),
        "i": placed_input(28, 90),
        "c": arrays_input(7, 100, 360, 12, 0.04, 60),
        "j_short": dict(placed_input(31, 60), q_range=(0, 7, 0)),
        "j_lower": empty,
    }


def long_input(seed, length, rate=0.01, flank=300, **more):
    """One segment of `length` bases in the query and, with substitutions at `rate`, in the reference, between random flanks:
    under a large max_sd_size the windows at its ends grow a hit across all of it."""
    rng = np.random.default_rng(seed)
    seg = rng.integers(0, 4, length)
    qs = LETTERS[np.concatenate([rng.integers(0, 4, flank), seg, rng.integers(0, 4, flank)])].tobytes()
    rs = LETTERS[np.concatenate([rng.integers(0, 4, flank), tandem(rng, seg, 1, rate), rng.integers(0, 4, flank)])].tobytes()
    I = dict(pool=qs + rs, q_range=(0, len(qs), 0), r_range=(len(qs), len(rs), 0), same_genome=0, init_len=60, k=8, w=4,
             limit=[max(1, s // 8) for s in range(8192)], max_sd_size=1 << 20)  # (a table for the sizes a long hit's query reaches)
    I.update(more)
    return I


def copies_input(seed, length, copies, rate=0.01, flank=300, gap=300):
    """long_input's query against a reference with `copies` copies of the segment, random stretches between them: the window
    at the segment's start grows one long hit per copy."""
    rng = np.random.default_rng(seed)
    seg = rng.integers(0, 4, length)
    qs = LETTERS[np.concatenate([rng.integers(0, 4, flank), seg, rng.integers(0, 4, flank)])].tobytes()
    parts = [rng.integers(0, 4, flank)]
    for _ in range(copies):
        parts += [tandem(rng, seg, 1, rate), rng.integers(0, 4, gap)]
    rs = LETTERS[np.concatenate(parts)].tobytes()
    return dict(pool=qs + rs, q_range=(0, len(qs), 0), r_range=(len(qs), len(rs), 0), same_genome=0, init_len=60, k=8, w=4,
                limit=[max(1, s // 8) for s in range(8192)], max_sd_size=1 << 20)
