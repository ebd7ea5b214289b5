"""Search seeding as include/sedef_hip.h states it (sdf_search_windows): the front half of the reference's search()
(src/search.cc:395-452) with an empty tree, for every query minimizer, in plain Python on numpy arrays.  The loops are the
reference's, written out; nothing here is in closed form."""
import numpy as np

MINIMIZER = np.dtype([("hash", "<u4"), ("loc", "<i4"), ("status", "<i4"), ("range", "<i4")])
WINDOW = np.dtype([("query_size", "<i4"), ("n_members", "<i4"), ("n_gathered", "<i4"), ("n_candidates", "<i4"), ("flags", "<u4")])
INTERVAL = np.dtype([("start", "<i4"), ("end", "<i4")])
SHORT, NOLIMIT, WIDE = 1, 2, 4
MAX_MEMBERS, MAX_GATHER = 1024, 4096


def records(rows):
    """(hash, loc, status) rows as minimizer records."""
    rows = np.asarray(rows, np.int64).reshape(-1, 3)
    out = np.zeros(len(rows), MINIMIZER)
    out["hash"], out["loc"], out["status"] = rows[:, 0], rows[:, 1], rows[:, 2]
    return out


def index_order(recs):
    """Records in the index's order: ascending (status, hash, loc)."""
    return recs[np.lexsort((recs["loc"], recs["hash"], recs["status"]))]


def keys_of(recs):
    return recs["status"].astype(np.uint32).astype(np.uint64) << np.uint64(32) | recs["hash"].astype(np.uint64)


def window(qloc, qstatus, qkeys, i, r_locs, groups, r_threshold, len_q, init_len, same_genome, uppercase_seeds, limit):
    """Window i: (query_size, n_members, n_gathered, candidates, flags, intervals).  qloc, qstatus, qkeys, r_locs: lists;
    groups: per query minimizer the run [g0, g1) of the reference's records with its key."""
    qs = qloc[i]
    if qs + init_len > len_q:
        return 0, 0, 0, [], SHORT, []
    seen, cand, gathered, j = set(), set(), 0, i
    while j < len(qloc) and qloc[j] - qs <= init_len:
        seen.add(qkeys[j])
        if not uppercase_seeds or qstatus[j] == 0:
            g0, g1 = groups[j]
            if g0 < g1 and g1 - g0 < r_threshold:
                gathered += g1 - g0
                for pos in r_locs[g0:g1]:
                    if not same_genome or pos >= qs + init_len:
                        cand.add(pos)
        j += 1
    n_members, query_size = j - i, len(seen)
    flags = WIDE if n_members > MAX_MEMBERS or gathered > MAX_GATHER else 0
    c = sorted(cand)
    if query_size >= len(limit):
        return query_size, n_members, gathered, c, flags | NOLIMIT, []
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


def search_windows(q, r_sorted, r_threshold, len_q, init_len, same_genome, uppercase_seeds, limit, device=False, detail=False):
    """(first, windows, intervals) as sdf_search_windows answers; device=True: as sdf_search_windows_device does (a WIDE
    window keeps its counts except n_candidates and has no interval).  detail=True: the candidates of every window behind them."""
    qkeys, rkeys = keys_of(q), keys_of(r_sorted)
    assert np.all(np.diff(q["loc"].astype(np.int64)) >= 0) and np.all(rkeys[1:] >= rkeys[:-1])
    r_locs, qloc, qstatus = r_sorted["loc"].tolist(), q["loc"].tolist(), q["status"].tolist()
    groups = np.stack([np.searchsorted(rkeys, qkeys, "left"), np.searchsorted(rkeys, qkeys, "right")], 1).tolist()
    qkeys = qkeys.tolist()
    windows, first, out, cands = np.zeros(len(q), WINDOW), [0], [], []
    for i in range(len(q)):
        qsz, nm, ng, c, flags, T = window(qloc, qstatus, qkeys, i, r_locs, groups, r_threshold, len_q, init_len, same_genome, uppercase_seeds,
                                          limit)
        if device and flags & WIDE:
            c, T = [], []
        windows[i] = (qsz, nm, min(ng, 2 ** 31 - 1), len(c), flags)
        out += T
        cands.append(c)
        first.append(len(out))
    res = (np.array(first, np.int64), windows, np.array(out, np.int64).reshape(-1, 2).astype("<i4").view(INTERVAL).reshape(-1))
    return res + (cands,) if detail else res
