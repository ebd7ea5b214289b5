"""The search extension as include/sedef_hip.h states it (sdf_search_extend): the reference's extend() (src/search.cc:95-259)
for every rolled interval, in plain Python.  The state is roll_model.Sliding -- a dict of bits, the sorted stored keys, B and
I -- with the query side's two operations and query_size beside it; the walk of the roll is replayed one base a step up to
the evaluation that assigned its best, and the extension does and undoes its steps in the reference's order."""
import bisect
import math

import numpy as np

import roll_model as R

HIT = np.dtype([("query_start", "<i4"), ("query_end", "<i4"), ("ref_start", "<i4"), ("ref_end", "<i4"), ("jaccard", "<i4"),
                ("q_winnow_start", "<i4"), ("q_winnow_end", "<i4"), ("r_winnow_start", "<i4"), ("r_winnow_end", "<i4"),
                ("flags", "<u4")])
SKIPPED, WIDE, NOLIMIT = 1, 2, 4
MAX_GROW = 1792
FILTER_STOPS = 1 | 2 | 8  # UPPER_FAIL | QGRAM_FAIL | SKIPPED
DEFAULTS = dict(max_error=0.30, max_edit_error=0.15, max_sd_size=1 << 20, same_genome=0)
COUNTERS = ("undos", "false_add_undos", "stop_len", "stop_ratio", "stop_overlap", "at_end", "guards")


class NoLimit(Exception):
    pass


class Sliding(R.Sliding):
    """roll_model.Sliding (add and remove of the reference side, as the roll uses them) and the four operations of the
    extension: B may be None, query_size is counted and L follows it."""

    def __init__(self, member_keys, query_size, limit, seen=None):
        R.Sliding.__init__(self, member_keys, int(limit[query_size]), seen)
        self.query_size, self.limit = query_size, limit

    def below(self, key):
        at = bisect.bisect_left(self.keys, key)
        return self.keys[at - 1] if at else None

    def above(self, key):
        at = bisect.bisect_right(self.keys, key)
        return self.keys[at] if at < len(self.keys) else None

    def full(self, key):
        return self.bits.get(key, 0) == 3

    def add_bit(self, key, bit):
        b = self.bits.get(key, 0)
        if b & bit:
            return False
        self.bits[key] = b | bit
        if b == 0:
            bisect.insort(self.keys, key)
        if self.query_size and self.B is None:
            self.count("guards")
        if self.query_size and self.B is not None and key < self.B:
            self.I += (b | bit) == 3
            if b == 0:
                self.I -= self.full(self.B)
                self.B = self.below(self.B)
        return True

    def remove_bit(self, key, bit):
        b = self.bits.get(key, 0)
        if not b & bit:
            if self.above(key) is None and not b:
                self.count("guards")  # (lower_bound(key) == end())
            return False
        if self.query_size and self.B is None:
            self.count("guards")
        if self.query_size and self.B is not None and key <= self.B:
            self.I -= b == 3
            if b == bit:
                up = self.above(self.B)
                if up is None:
                    self.count("guards")
                else:
                    self.B = up
                    self.I += self.full(self.B)
        if b == bit:
            del self.bits[key]
            self.keys.pop(bisect.bisect_left(self.keys, key))
        else:
            self.bits[key] = b & ~bit
        return True

    def relimit(self, size):
        if size >= len(self.limit):
            raise NoLimit
        self.query_size, self.L = size, int(self.limit[size])

    def add_to_query(self, key):
        if not self.add_bit(key, 1):
            return False
        self.relimit(self.query_size + 1)
        if self.B is None:
            self.B = self.keys[0]
        else:
            up = self.above(self.B)
            if up is None:
                self.count("guards")
            else:
                self.B = up
        self.I += self.full(self.B)
        return True

    def remove_from_query(self, key):
        if not self.remove_bit(key, 1):
            return
        self.relimit(max(0, self.query_size - 1))
        if self.B is not None:
            self.I -= self.full(self.B)
            self.B = self.below(self.B)

    def add_to_reference(self, key, status):
        if status != 2:
            self.add_bit(key, 2)

    def remove_from_reference(self, key, status):
        if status != 2:
            self.remove_bit(key, 2)


def replay(S, start, end, r_loc, r_key, r_status, len_r, init_len, rws, rwe):
    """The roll's walk on S up to the first evaluation of J with ws >= rws and we >= rwe (or to its end)."""
    nr = len(r_loc)
    s, e = start, min(start + init_len, len_r)
    ws = bisect.bisect_left(r_loc, s)
    we = ws
    while we < nr and r_loc[we] < e:
        S.add(r_key[we], r_status[we])
        we += 1
    while not (ws >= rws and we >= rwe) and s < end and e < len_r:
        if ws < nr and r_loc[ws] <= s:
            S.remove(r_key[ws], r_status[ws])
            ws += 1
        if we < nr and r_loc[we] == e:
            S.add(r_key[we], r_status[we])
            we += 1
        s += 1
        e += 1


def pct(p, tot):
    p, tot = float(p), float(tot)
    if tot == 0.0:
        return math.nan if p == 0.0 else math.copysign(math.inf, p)
    return 100.0 * p / tot


def to_int(v):
    return 0 if v != v else 2147483647 if v >= 2147483647.0 else -2147483648 if v <= -2147483648.0 else int(v)


def extend(S, q_loc, q_key, r_loc, r_key, r_status, len_q, len_r, qws, qwe, rws, rwe, P, seen, stop_when_wide=False):
    """One interval from its entry state: (query_start .. r_winnow_end), or None when an add needed the limit table beyond its
    end, and whether a step went beyond MAX_GROW.  stop_when_wide: as the kernel does, end at that step, before its adds."""
    grown = [False]
    try:
        return extend_rounds(S, q_loc, q_key, r_loc, r_key, r_status, len_q, len_r, qws, qwe, rws, rwe, P, seen, stop_when_wide, grown)
    except NoLimit:
        return None, grown[0]


def extend_rounds(S, q_loc, q_key, r_loc, r_key, r_status, len_q, len_r, qws, qwe, rws, rwe, P, seen, stop_when_wide, grown):
    nq, nr = len(q_loc), len(r_loc)
    entry = (qws, qwe, rws, rwe)
    wide = False
    qs = q_loc[qws - 1] + 1 if qws else 0
    qe = q_loc[qwe] if qwe < nq else len_q
    rs = r_loc[rws - 1] + 1 if rws else 0
    re = r_loc[rwe] if rwe < nr else len_r
    gap = P["max_error"] - P["max_edit_error"]
    while True:
        max_match = P["max_sd_size"]
        if P["same_genome"]:
            max_match = min(max_match, to_int((1.0 / gap + .5) * abs(qs - rs)))
        aln_len, seq_len = max(qe - qs, re - rs), min(qe - qs, re - rs)
        if aln_len > max_match:
            seen["stop_len"] = seen.get("stop_len", 0) + 1
            break
        if pct(seq_len, aln_len) < 100 * (1 - 2 * gap):
            seen["stop_ratio"] = seen.get("stop_ratio", 0) + 1
            break
        if P["same_genome"] and qe - rs > 0 and pct(qe - rs, re - rs) > 100 * P["max_error"]:
            seen["stop_overlap"] = seen.get("stop_overlap", 0) + 1
            break
        extended = False
        for left, right in ((True, True), (False, True), (True, False)):  # both_both, both_right, both_left
            if left and (not qws or not rws):
                continue
            if right and (rwe >= nr or qwe >= nq):
                continue
            false_add = False
            # the growth cap, for every side of the step before its first add
            wide |= left and (entry[0] - qws >= MAX_GROW or entry[2] - rws >= MAX_GROW)
            wide |= right and (qwe - entry[1] >= MAX_GROW or rwe - entry[3] >= MAX_GROW)
            grown[0] = wide
            if wide and stop_when_wide:
                return None, True
            if left:
                qws -= 1
                false_add |= not S.add_to_query(q_key[qws])
                qs = q_loc[qws - 1] + 1 if qws else 0
                rws -= 1
                S.add_to_reference(r_key[rws], r_status[rws])
                rs = r_loc[rws - 1] + 1 if rws else 0
            if right:
                false_add |= not S.add_to_query(q_key[qwe])
                qwe += 1
                qe = q_loc[qwe] if qwe < nq else len_q
                S.add_to_reference(r_key[rwe], r_status[rwe])
                rwe += 1
                re = r_loc[rwe] if rwe < nr else len_r
            if S.jaccard() >= 0:
                extended = True
                break
            seen["undos"] = seen.get("undos", 0) + 1
            seen["false_add_undos"] = seen.get("false_add_undos", 0) + false_add
            if right:  # the reference's undo: removes, not a restore
                rwe -= 1
                S.remove_from_reference(r_key[rwe], r_status[rwe])
                re = r_loc[rwe]
                qwe -= 1
                S.remove_from_query(q_key[qwe])
                qe = q_loc[qwe]
            if left:
                rs = r_loc[rws] + 1
                S.remove_from_reference(r_key[rws], r_status[rws])
                rws += 1
                qs = q_loc[qws] + 1
                S.remove_from_query(q_key[qws])
                qws += 1
        if not extended:
            break
    seen["at_end"] = seen.get("at_end", 0) + (not qws or not rws or qwe == nq or rwe == nr)
    return (qs, qe, rs, re, S.jaccard(), qws, qwe, rws, rwe), wide


def search_extend(q, windows, first, intervals, r, len_r, init_len, limit, rolls, len_q, filt=None, params=None, device=False,
                  seen=None):
    """The records of sdf_search_extend; device=True: as sdf_search_extend_device writes them (a WIDE interval is flagged, the
    rest of its record zero).  seen: a dict that counts the quirks met."""
    P = dict(DEFAULTS, **(params or {}))
    seen = seen if seen is not None else {}
    out = np.zeros(int(first[-1]), HIT)
    qk, rk = R.keys_of(q), R.keys_of(r)
    q_loc, r_loc, r_status = q["loc"].tolist(), r["loc"].tolist(), r["status"].tolist()
    limit = [int(x) for x in limit]
    for i in range(len(q)):
        nm = int(windows["n_members"][i])
        for t in range(int(first[i]), int(first[i + 1])):
            roll = rolls[t]
            start, end = int(intervals["start"][t]), int(intervals["end"][t])
            lo = bisect.bisect_left(r_loc, start)
            rws, rwe = int(roll["winnow_start"]), int(roll["winnow_end"])
            runs = roll["jaccard"] >= 0 and not roll["flags"] & R.BADWINDOW and not (roll["flags"] & R.WIDE and roll["ref_end"] == 0)
            runs = runs and (filt is None or not filt["flags"][t] & FILTER_STOPS) and lo <= rws <= rwe <= len(r)
            if not runs:
                out[t]["flags"] = SKIPPED
                continue
            wide = bool(roll["flags"] & R.WIDE) or nm > R.MAX_MEMBERS or rwe - lo > R.MAX_SPAN
            if device and wide:
                out[t]["flags"] = WIDE
                continue
            S = Sliding(qk[i:i + nm], int(windows["query_size"][i]), limit, seen)
            replay(S, start, end, r_loc, rk, r_status, len_r, init_len, rws, rwe)
            hit, grew = extend(S, q_loc, qk, r_loc, rk, r_status, len_q, len_r, i, i + nm, rws, rwe, P, seen, stop_when_wide=device)
            if device and grew:
                out[t]["flags"] = WIDE
            elif hit is None:
                out[t]["flags"] = NOLIMIT | (WIDE if wide or grew else 0)
            else:
                out[t] = hit + (WIDE if wide or grew else 0,)
    return out


def hit_task(hit, len_q, len_r, q_off, q_rc, r_off, r_rc):
    """The filter task of a hit (sdf_search_hit_tasks_*): (q_off, r_off, q_len, r_len, flags, 0)."""
    qa, qb, ra, rb = (int(hit[name]) for name in ("query_start", "query_end", "ref_start", "ref_end"))
    if hit["flags"] & (SKIPPED | NOLIMIT) or (hit["flags"] & WIDE and qb == 0) or not (0 <= qa <= qb <= len_q and 0 <= ra <= rb <= len_r):
        return (0, 0, 0, 0, 4, 0)
    return (q_off + len_q - qb if q_rc else q_off + qa, r_off + len_r - rb if r_rc else r_off + ra, qb - qa, rb - ra,
            (1 if q_rc else 0) | (2 if r_rc else 0), 0)
