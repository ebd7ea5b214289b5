"""The search filter as include/sedef_hip.h states it (sdf_search_filter), in a dozen lines of numpy: what the kernel and
sdf_search_filter_host are compared with where the fixture ends.  Also the task of a rolled interval
(sdf_search_filter_tasks_*)."""
import numpy as np

TASK = np.dtype([("q_off", "<i8"), ("r_off", "<i8"), ("q_len", "<i4"), ("r_len", "<i4"), ("flags", "<u4"), ("reserved", "<i4")])
REC = np.dtype([("q_up", "<i4"), ("r_up", "<i4"), ("dist", "<i4"), ("minqg", "<i4"), ("flags", "<u4")])
Q_RC, R_RC, SKIP = 1, 2, 4
UPPER_FAIL, QGRAM_FAIL, SHORT, SKIPPED = 1, 2, 4, 8
ROLL_WIDE, ROLL_BADWINDOW, WINDOW_SHORT, WINDOW_NOLIMIT = 1, 2, 1, 2
DEFAULTS = dict(min_uppercase=12, max_error=0.30, max_edit_error=0.15, gap_frequency=0.005)

_REV = np.full(128, ord("N"), np.uint8)
_REV[list(b"ACGTacgt")] = list(b"TGCAtgca")
_CODE = np.zeros(128, np.int64)
_CODE[list(b"CGTcgt")] = [1, 2, 3, 1, 2, 3]


def side(pool, off, length, rc):
    """The characters of a side: pool[off, off + length) & 127, reverse-complemented by rev_dna when rc."""
    s = np.frombuffer(pool, np.uint8, length, off) & 127
    return _REV[s[::-1]] if rc else s


def grams(s):
    """The count of each of the 1,024 5-grams of s."""
    c = _CODE[s]
    if len(c) < 5:
        return np.zeros(1024, np.int64)
    return np.bincount(c[:-4] * 256 + c[1:-3] * 64 + c[2:-2] * 16 + c[3:-1] * 4 + c[4:], minlength=1024)


def minqg(l, max_error, max_edit_error, gap_frequency, **_):
    """(python floats are IEEE doubles and nothing fuses: the association is the header's)"""
    return int(l * (1 - (max_error - max_edit_error) - 5 * max_edit_error) - (gap_frequency * l + 1) * 4)


def filter_pairs(pool, tasks, **params):
    P = dict(DEFAULTS, **params)
    out = np.zeros(len(tasks), REC)
    for t, T in enumerate(tasks):
        if int(T["flags"]) & SKIP:
            out[t]["flags"] = SKIPPED
            continue
        q = side(pool, int(T["q_off"]), int(T["q_len"]), int(T["flags"]) & Q_RC)
        r = side(pool, int(T["r_off"]), int(T["r_len"]), int(T["flags"]) & R_RC)
        q_up, r_up = (int(((x >= 65) & (x <= 90)).sum()) for x in (q, r))
        dist, m = int(np.minimum(grams(q), grams(r)).sum()), minqg(max(len(q), len(r)), **P)
        flags = UPPER_FAIL if min(q_up, r_up) < P["min_uppercase"] else QGRAM_FAIL if dist < m else 0
        out[t] = (q_up, r_up, dist, m, flags | (SHORT if m < 10 else 0))
    return out


def filter_tasks(q, windows, first, intervals, rolls, len_q, len_r, init_len, q_off, q_rc, r_off, r_rc, allow_extend):
    """out[t] for every rolled interval t: the query window against the roll's best range, or -- allow_extend -- against the
    range where the walk ended."""
    out = np.zeros(int(first[-1]), TASK)
    for i in range(len(q)):
        for t in range(int(first[i]), int(first[i + 1])):
            R, T = rolls[t], intervals[t]
            qa, qb, ra, rb = int(q[i]["loc"]), int(q[i]["loc"]) + init_len, int(R["ref_start"]), int(R["ref_end"])
            if allow_extend:
                start, end = int(T["start"]), int(T["end"])
                e0 = min(start + init_len, len_r)
                steps = max(0, min(end - start, len_r - e0))
                ra, rb = start + steps, e0 + steps
            skip = int(R["jaccard"]) < 0 or int(R["flags"]) & ROLL_BADWINDOW or (int(R["flags"]) & ROLL_WIDE and int(R["ref_end"]) == 0) \
                or int(windows[i]["flags"]) & (WINDOW_SHORT | WINDOW_NOLIMIT) or qa < 0 or qb > len_q or ra < 0 or rb < ra or rb > len_r
            if skip:
                out[t]["flags"] = SKIP
                continue
            out[t] = (q_off + len_q - qb if q_rc else q_off + qa, r_off + len_r - rb if r_rc else r_off + ra, qb - qa, rb - ra,
                      (Q_RC if q_rc else 0) | (R_RC if r_rc else 0), 0)
    return out
