"""The search roll as include/sedef_hip.h states it (sdf_search_roll): the first loop of the reference's
search_in_reference_interval (src/search.cc:274-314) for every interval of search_windows, in plain Python.  The state is a
dict of bits and a sorted list of the stored keys; the walk takes every base as a step of its own, nothing is skipped."""
import bisect

import numpy as np

ROLL = np.dtype([("ref_start", "<i4"), ("ref_end", "<i4"), ("winnow_start", "<i4"), ("winnow_end", "<i4"), ("jaccard", "<i4"),
                 ("flags", "<u4")])
WIDE, BADWINDOW = 1, 2
MAX_MEMBERS, MAX_SPAN = 1024, 3072
COUNTERS = ("dup_removes", "adds_on_boundary", "negative", "status2", "clamped", "ended_at_len_r")


class Sliding:
    """bits[key] (1: query, 2: reference), the sorted stored keys, the boundary key B and the counter I."""

    def __init__(self, member_keys, limit, seen=None):
        self.bits = {k: 1 for k in member_keys}
        self.keys = sorted(self.bits)
        self.B = self.keys[-1]
        self.I = 0
        self.L = limit
        self.seen = seen if seen is not None else {}

    def count(self, what):
        self.seen[what] = self.seen.get(what, 0) + 1

    def add(self, key, status):
        if status == 2:
            return
        b = self.bits.get(key, 0)
        if b & 2:
            return
        if key == self.B:
            self.count("adds_on_boundary")
        if b == 1:
            self.bits[key] = 3
            if key < self.B:
                self.I += 1
            return
        self.bits[key] = 2
        bisect.insort(self.keys, key)
        if key < self.B:
            self.I -= self.bits[self.B] == 3
            self.B = self.keys[bisect.bisect_left(self.keys, self.B) - 1]

    def remove(self, key, status):
        if status == 2:
            return
        b = self.bits.get(key, 0)
        if not b & 2:
            self.count("dup_removes")
            return
        if key <= self.B:
            self.I -= b == 3
            if b == 2:
                self.B = self.keys[bisect.bisect_right(self.keys, self.B)]
                self.I += self.bits[self.B] == 3
        if b == 2:
            del self.bits[key]
            self.keys.pop(bisect.bisect_left(self.keys, key))
        else:
            self.bits[key] = 1

    def jaccard(self):
        if self.I < 0:
            self.seen["negative"] = 1
        return self.I if self.I >= self.L else self.I - self.L


def roll(member_keys, L, start, end, r_loc, r_key, r_status, len_r, init_len, seen=None):
    """One interval: (ref_start, ref_end, winnow_start, winnow_end, jaccard).  r_loc, r_key, r_status: lists in loc order."""
    S = Sliding(member_keys, L, seen)
    nr = len(r_loc)
    s, e = start, min(start + init_len, len_r)
    ws = bisect.bisect_left(r_loc, s)
    we = ws
    while we < nr and r_loc[we] < e:
        S.add(r_key[we], r_status[we])
        we += 1
    best = (s, e, ws, we, S.jaccard())
    while s < end and e < len_r:
        if ws < nr and r_loc[ws] <= s:
            S.remove(r_key[ws], r_status[ws])
            ws += 1
        if we < nr and r_loc[we] == e:
            S.add(r_key[we], r_status[we])
            we += 1
        j = S.jaccard()
        if j > best[4]:
            best = (s, e, ws, we, j)
        s += 1
        e += 1
    return best


def keys_of(recs):
    return (recs["status"].astype(np.uint32).astype(np.uint64) << np.uint64(32) | recs["hash"].astype(np.uint64)).tolist()


def search_roll(q, windows, first, intervals, r, len_r, init_len, limit, device=False, seen=None):
    """The records of sdf_search_roll; device=True: as sdf_search_roll_device writes them (a WIDE interval is flagged, the
    rest of its record zero).  seen: a dict that counts the quirks met."""
    out = np.zeros(int(first[-1]), ROLL)
    qk, rk = keys_of(q), keys_of(r)
    r_loc, r_status = r["loc"].tolist(), r["status"].tolist()
    for i in range(len(q)):
        nm = int(windows["n_members"][i])
        for t in range(int(first[i]), int(first[i + 1])):
            start, end = int(intervals["start"][t]), int(intervals["end"][t])
            span = bisect.bisect_right(r_loc, end + init_len) - bisect.bisect_left(r_loc, start)
            flags = WIDE if nm > MAX_MEMBERS or span > MAX_SPAN else 0
            if device and flags:
                out[t] = (0, 0, 0, 0, 0, flags)
                continue
            out[t] = roll(qk[i:i + nm], int(limit[int(windows["query_size"][i])]), start, end, r_loc, rk, r_status, len_r,
                          init_len, seen) + (flags,)
    return out
