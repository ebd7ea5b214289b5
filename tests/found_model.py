"""The two tree queries of the reference's search (src/search.cc:420-434 and is_overlap, :35-71) as include/sedef_hip.h
states them for sdf_search_windows_found and sdf_search_overlap -- twice, independently:

  the record-list model   the header's definitions as brute force over found[:visible];
  the point-level model   the reference's Tree as Boost.ICL documents it, point by point: a dict from query base to a dict from
                          reference base to a set of (a, b) -- what an interval_map of interval_maps that aggregates by set union
                          holds at every point.  "add hit" loops over every point of a and every point of b, find() is a lookup,
                          `tree -= [0, x)` deletes the points below x; search()'s exclusion and is_overlap are transcribed line
                          by line on it.  Only usable on sequences of a few kilobases with a handful of hits.

Both share the window walk (search_model.window's, with a hook where the reference asks the tree): the difference between the
two models is what answers the hook."""
import numpy as np

import search_model as S

FOUND = np.dtype([("q_start", "<i4"), ("q_end", "<i4"), ("r_start", "<i4"), ("r_end", "<i4")])
FOUND_WIDE, MAX_FOUND, BIN_SHIFT = 8, 256, 12


def found_records(rows):
    """(q_start, q_end, r_start, r_end) rows as found records."""
    rows = np.asarray(rows, np.int64).reshape(-1, 4)
    out = np.zeros(len(rows), FOUND)
    for k, f in enumerate(FOUND.names):
        out[f] = rows[:, k]
    return out


def rows_of(found):
    return [tuple(int(x) for x in f) for f in np.asarray(found, FOUND).tolist()] if len(found) else []


# ---- the record-list model ----

def empty(R):
    return R[0] >= R[1] or R[2] >= R[3]


def covers(R, loc, pos):
    return R[0] <= loc < R[1] and R[2] <= pos < R[3]


class RecordList:
    """found[:visible] as a query sees it."""

    def __init__(self, rows, visible):
        self.rows = [R for R in rows[:visible] if not empty(R)]

    def excluded(self, loc, pos):
        return any(covers(R, loc, pos) for R in self.rows)

    def meeting(self, qs, init_len):
        """The records SDF_SEARCH_FOUND_WIDE counts: those that can contain the loc of a member of the window at qs."""
        return sum(1 for R in self.rows if R[0] <= qs + init_len and R[1] > qs)

    def is_overlap(self, pf_pos, pf_end, pfp_pos, pfp_end, min_read_size):
        for sA, eA, sB, eB in self.rows:
            if not covers((sA, eA, sB, eB), pf_pos, pfp_pos):
                continue
            if pf_pos >= sA and pf_end <= eA and pfp_pos >= sB and pfp_end <= eB:
                return True
            if min(eA - sA, eB - sB) < min_read_size * 1.5:
                continue
            if eA - pf_pos >= min_read_size and eB - pfp_pos >= min_read_size:
                return True
        return False


# ---- the point-level model of the ICL tree ----

class PointTree:
    """Tree = interval_map<int, Subtree>, Subtree = interval_map<int, set<pair<Interval, Interval>>>, both aggregating by set
    union, at every point."""

    def __init__(self):
        self.t = {}

    def add_hit(self, a, b):
        """tree += make_pair(a, Subtree({b, {make_pair(a, b)}})) for right-open a and b.  An empty b makes an empty Subtree,
        which ICL absorbs: no point of a appears; an empty a adds nothing."""
        for x in range(a[0], a[1]):
            for y in range(b[0], b[1]):
                sub = self.t.get(x)
                if sub is None:
                    sub = self.t[x] = {}
                at = sub.get(y)
                if at is None:
                    sub[y] = {(a, b)}
                else:
                    at.add((a, b))

    def trim(self, x):
        """tree -= Interval(0, x): right-open, nothing for x <= 0."""
        for p in [p for p in self.t if 0 <= p < x]:
            del self.t[p]

    def excluded(self, loc, pos):
        """src/search.cc:420, 431: pf = tree.find(loc); the position survives when pf == end or pf->second.find(pos) == end."""
        pf = self.t.get(loc)
        return not (pf is None or pf.get(pos) is None)

    def is_overlap(self, pf_pos, pf_end, pfp_pos, pfp_end, min_read_size):
        """src/search.cc:35-71, line by line."""
        assert pf_pos <= pf_end
        pf = self.t.get(pf_pos)
        if pf is None:
            return False
        pfp = pf.get(pfp_pos)
        if pfp is None:
            return False
        for (sA, eA), (sB, eB) in sorted(pfp):
            if pf_pos >= sA and pf_end <= eA and pfp_pos >= sB and pfp_end <= eB:
                return True
            if min(eA - sA, eB - sB) < min_read_size * 1.5:
                continue
            RIGHT_ALLOWANCE = min_read_size
            if eA - pf_pos >= RIGHT_ALLOWANCE and eB - pfp_pos >= RIGHT_ALLOWANCE:
                return True
        return False


# ---- the window walk, with a hook where the reference asks the tree ----

def window(qloc, qstatus, qkeys, i, r_locs, groups, r_threshold, len_q, init_len, same_genome, uppercase_seeds, limit, excluded):
    """search_model.window with the exclusion: (query_size, n_members, n_gathered, candidates, flags, intervals); flags
    without FOUND_WIDE.  excluded(loc, pos): the tree's answer for the member at loc."""
    qs = qloc[i]
    if qs + init_len > len_q:
        return 0, 0, 0, [], S.SHORT, []
    seen, cand, gathered, j = set(), set(), 0, i
    while j < len(qloc) and qloc[j] - qs <= init_len:
        seen.add(qkeys[j])
        if not uppercase_seeds or qstatus[j] == 0:
            g0, g1 = groups[j]
            if g0 < g1 and g1 - g0 < r_threshold:
                gathered += g1 - g0
                for pos in r_locs[g0:g1]:
                    if not same_genome or pos >= qs + init_len:
                        if not excluded(qloc[j], pos):
                            cand.add(pos)
        j += 1
    n_members, query_size = j - i, len(seen)
    flags = S.WIDE if n_members > S.MAX_MEMBERS or gathered > S.MAX_GATHER else 0
    c = sorted(cand)
    if query_size >= len(limit):
        return query_size, n_members, gathered, c, flags | S.NOLIMIT, []
    L = int(limit[query_size])
    T = []
    for a in range(0, len(c) - L + 1):
        b = a + L - 1
        if c[b] - c[a] <= init_len:
            x, y = max(0, c[b] - init_len + 1), c[a] + 1
            if T and x < T[-1][1]:
                T[-1][1] = max(T[-1][1], y)
            else:
                T.append([x, y])
    out = []
    for x, y in T:
        if same_genome:
            x = max(x, qs + init_len)
        if x > y:
            continue
        out.append((x, y))
    return query_size, n_members, gathered, c, flags, out


class Walker:
    """The arrays of a call, prepared once; window(i, excluded) walks one window."""

    def __init__(self, q, r_sorted, r_threshold, len_q, init_len, same_genome, uppercase_seeds, limit):
        qkeys, rkeys = S.keys_of(q), S.keys_of(r_sorted)
        self.r_locs, self.qloc, self.qstatus = r_sorted["loc"].tolist(), q["loc"].tolist(), q["status"].tolist()
        self.groups = np.stack([np.searchsorted(rkeys, qkeys, "left"), np.searchsorted(rkeys, qkeys, "right")], 1).tolist()
        self.qkeys = qkeys.tolist()
        self.tail = (r_threshold, len_q, init_len, same_genome, uppercase_seeds, limit)
        self.init_len = init_len

    def window(self, i, excluded):
        return window(self.qloc, self.qstatus, self.qkeys, i, self.r_locs, self.groups, *self.tail, excluded)


def search_windows_found(q, r_sorted, r_threshold, len_q, init_len, same_genome, uppercase_seeds, limit, found, visible, device=False):
    """(first, windows, intervals) as sdf_search_windows_found answers by the record-list model; device=True: as
    sdf_search_windows_found_device does (a WIDE or FOUND_WIDE window keeps its counts except n_candidates and has no
    interval)."""
    walk = Walker(q, r_sorted, r_threshold, len_q, init_len, same_genome, uppercase_seeds, limit)
    rows = rows_of(found)
    windows, first, out = np.zeros(len(q), S.WINDOW), [0], []
    for i in range(len(q)):
        see = RecordList(rows, int(visible[i]))
        qsz, nm, ng, c, flags, T = walk.window(i, see.excluded)
        if not flags & S.SHORT and see.meeting(walk.qloc[i], init_len) > MAX_FOUND:
            flags |= FOUND_WIDE
        if device and flags & (S.WIDE | FOUND_WIDE):
            c, T = [], []
        windows[i] = (qsz, nm, min(ng, 2 ** 31 - 1), len(c), flags)
        out += T
        first.append(len(out))
    return np.array(first, np.int64), windows, np.array(out, np.int64).reshape(-1, 2).astype("<i4").view(S.INTERVAL).reshape(-1)


def search_overlap(q, first, rolls, found, visible_iv, init_len, min_read_size):
    """The verdicts of sdf_search_overlap by the record-list model."""
    rows = rows_of(found)
    out = np.zeros(int(first[-1]), np.uint32)
    for i in range(len(q)):
        for t in range(int(first[i]), int(first[i + 1])):
            pf_pos = int(q["loc"][i])
            out[t] = RecordList(rows, int(visible_iv[t])).is_overlap(pf_pos, pf_pos + init_len, int(rolls["ref_start"][t]),
                                                                      int(rolls["ref_end"][t]), min_read_size)
    return out
