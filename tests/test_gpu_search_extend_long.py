"""The long form of the search extension on the device (sdf_search_extend_long_device; sedef_amd/csrc/search_extend_long.hip):
the intervals sdf_search_extend_device flags WIDE for their growth, completed in place up to long_grow records an end.

The truth is sdf_search_extend_host on the same arrays, record for record (tests/test_search_extend_cpu.py pins that form
against the reference, on short growths).  Every comparison is exact."""
import os
import sys

import numpy as np
import pytest
import torch  # (at collection: before the library brings a HIP runtime of its own along)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import extend_model as E  # noqa: E402
import minim_model as M  # noqa: E402
import roll_model as R  # noqa: E402
import search_model as S  # noqa: E402

pytestmark = pytest.mark.gpu

SDF_ERR_NOMEM, SDF_ERR_UNSUPPORTED, SDF_ERR_INVALID = -6, -3, -4
GUARD = 4  # records of 0xEE behind d_hits[n_max]
ZERO_WIDE = (0,) * 9 + (E.WIDE,)


@pytest.fixture(scope="module")
def eng():
    import sedef_amd
    e = sedef_amd.Extz2Engine(0)
    yield e
    e.close()


def up(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy() if len(a) else np.zeros(8, np.uint8)).cuda()


def host(args, params):
    from sedef_amd import extz2
    code, hits = extz2.search_extend_host(*args, extz2.extend_params(**params))
    assert code == 0
    return hits


def same_hits(got, want, what=""):
    assert got.tobytes() == want.tobytes(), (what, [(int(t), got[t], want[t]) for t in np.flatnonzero(got != want)[:5]])


class Uploaded:
    """The arrays of one input in HBM, and the two device forms on them."""

    def __init__(self, eng, args, params):
        from sedef_amd import extz2
        q, windows, first, intervals, rolls, filt, r, len_q, len_r, init_len, limit = args
        self.eng, self.n, self.params = eng, int(first[-1]), extz2.extend_params(**params)
        self.keep = [up(q), up(windows), up(np.asarray(first, np.uint64)), up(intervals), up(np.ascontiguousarray(rolls, extz2.SEARCH_ROLL_DTYPE)),
                     up(r), up(np.asarray(limit, np.int32))]
        self.filt = None if filt is None else up(np.ascontiguousarray(filt, extz2.FILTER_REC_DTYPE))
        d = self.keep
        self.head = (d[0].data_ptr(), len(q), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(),
                     None if self.filt is None else self.filt.data_ptr())
        self.tail = (d[5].data_ptr(), len(r), len_q, len_r, init_len, d[6].data_ptr(), len(limit))
        self.d_hits = torch.full(((self.n + GUARD) * 40,), 0xEE, dtype=torch.uint8, device="cuda")
        self.d_left = torch.full((2,), 77, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()  # (the tensors were filled on torch's stream)

    def short(self, stream=None):
        self.eng.search_extend_device(*self.head, self.n, *self.tail, self.d_hits.data_ptr(), self.params, stream=stream)

    def long(self, long_grow, n_long_max=None, batch=0, stream=None, check=True, n_max=None, left=True):
        return self.eng.search_extend_long_device(*self.head, self.n if n_max is None else n_max, *self.tail, self.d_hits.data_ptr(),
                                                  long_grow, n_long_max, batch, self.d_left.data_ptr() if left else None, self.params,
                                                  stream=stream, check=check)

    def hits(self):
        raw = self.d_hits.cpu().numpy().tobytes()
        assert raw[40 * self.n:] == b"\xEE" * (40 * GUARD)
        return np.frombuffer(raw[:40 * self.n], E.HIT)

    def left(self):
        got = self.d_left.cpu().numpy()
        assert got[1] == 77
        return int(got[0])


def as_short(want):
    """What sdf_search_extend_device writes where the host form writes `want`."""
    expect = want.copy()
    expect[(want["flags"] & E.WIDE) != 0] = ZERO_WIDE
    return expect


def grown(args, hits, t):
    """By how many records the four ends of interval t's winnow ranges moved beyond their entry values."""
    q, windows, first, intervals, rolls = args[:5]
    i = int(np.searchsorted(first, t, "right")) - 1
    h = hits[t]
    return (int(i - h["q_winnow_start"]), int(h["q_winnow_end"] - (i + windows["n_members"][i])), int(rolls["winnow_start"][t] - h["r_winnow_start"]),
            int(h["r_winnow_end"] - rolls["winnow_end"][t]))


@pytest.fixture(scope="module")
def records():
    """The minimizers of one random sequence at k = 3, w = 2: a record every base or two."""
    seq = bytes(np.random.default_rng(5).choice(np.frombuffer(b"ACGT", np.uint8), 13000))
    return S.records(M.get_minimizers(seq, 3, 2, True))


def members_end(records, i, init_len=12):
    return int(np.searchsorted(records["loc"], records["loc"][i] + init_len, "right"))


def identical_sequences(records, count, at, init_len=12):
    """Two identical sequences, cut behind `count` records (by records, not bases: the growth moves by exactly one record with
    count), and one interval for each window of `at`, where the window lies in the reference."""
    q = records[:count].copy()
    n_bases = int(q["loc"][-1]) + 3
    windows = np.zeros(len(q), S.WINDOW)
    windows["n_members"], windows["query_size"] = 1, 1
    first = np.zeros(len(q) + 1, np.int64)
    rows = []
    for i in sorted(at):
        nm = members_end(q, i, init_len) - i
        windows[i] = (len(set(R.keys_of(q[i:i + nm]))), nm, 0, 0, 0)
        first[i + 1:] += 1
        rows.append((q["loc"][i], q["loc"][i] + 1))
    intervals = np.array(rows, S.INTERVAL)
    limit = np.maximum(1, np.arange(400) // 4).astype(np.int32)
    rolls = R.search_roll(q, windows, first, intervals, q, n_bases, init_len, limit)
    return q, windows, first, intervals, rolls, None, q, n_bases, n_bases, init_len, limit


LONG = 2048  # the long_grow of the small cases
LONG_MAX = 16384  # SDF_EXTEND_LONG_MAX_GROW


@pytest.fixture(scope="module")
def two_growths(records):
    """(args, host hits) with growths of exactly 1,793 and exactly LONG, and the same one record longer: 1,793 and LONG + 1."""
    from sedef_amd import extz2
    ia, ib = extz2.EXTEND_MAX_GROW + 1, 1500  # a grows most to the left: by ia; b to the right: by count - its members' end
    out = []
    for over in (0, 1):
        args = identical_sequences(records, members_end(records, ib) + LONG + over, (ia, ib))
        hits = host(args, {})
        assert (hits["q_winnow_start"] == 0).all() and (hits["q_winnow_end"] == len(args[0])).all(), "the extensions reach both ends"
        assert max(grown(args, hits, 1)) == ia and max(grown(args, hits, 0)) == LONG + over  # (t = 0: window ib, the lower one)
        assert hits["flags"].tolist() == [E.WIDE, E.WIDE]
        out.append((args, hits))
    return out


def test_growth_of_1793_and_of_long_grow_and_one_more(eng, two_growths):
    (args, want), (args_over, want_over) = two_growths
    u = Uploaded(eng, args, {})
    u.short()
    same_hits(u.hits(), as_short(want), "short form")
    u.long(LONG)
    same_hits(u.hits(), want, "growth 1,793 and long_grow")
    assert u.left() == 0
    u = Uploaded(eng, args_over, {})
    u.short()
    u.long(LONG)
    got = u.hits()
    assert got[0].tolist() == ZERO_WIDE and got[1].tobytes() == want_over[1].tobytes() and u.left() == 1
    u.long(LONG + 1)  # the same records once more: the completed one is no candidate any more
    same_hits(u.hits(), want_over, "long_grow + 1")
    assert u.left() == 0


def test_the_fixture_through_the_long_form(eng):
    """tests/golden/search_extend_long_kat.json.gz: the reference's own hits on growths beyond 1,792 records, through the short
    form and then the long one.  (The reference knows no WIDE flag; tests/test_search_extend_long_cpu.py pins the host form,
    flag and all, on the same cases.)"""
    from test_search_extend_long_cpu import case_expected, case_extend_inputs, load_fixture, without_wide
    n = 0
    for c in load_fixture()["cases"]:
        args, params = case_extend_inputs(c)
        want = host(args, params)
        u = Uploaded(eng, args, params)
        u.short()
        same_hits(u.hits(), as_short(want), c["name"])
        n += int((u.hits()["flags"] == E.WIDE).sum())
        u.long(2 * LONG)  # (the widest growth of the fixture is some 2,300 records)
        got = u.hits()
        same_hits(without_wide(got), case_expected(c), c["name"])
        same_hits(got, want, c["name"])
        assert u.left() == 0
    assert n >= 20


def mutated(rng, seq, rate):
    a = np.frombuffer(seq, np.uint8).copy()
    at = np.flatnonzero(rng.random(len(a)) < rate)
    a[at] = np.frombuffer(b"ACGT", np.uint8)[(np.searchsorted(np.frombuffer(b"ACGT", np.uint8), a[at]) + rng.integers(1, 4, len(at))) % 4]
    return a.tobytes()


def test_one_interval_at_the_largest_long_grow(eng):
    """k = 12, w = 16 on 0.66 Mb a side, random, the reference unrelated to the query but for 152 kb to the left of the window
    (the query's at 7 % divergence) and 1.5 kb to its right.  The walk goes on in both directions until the length stop
    (max_sd_size = 330,000) ends it, some 9,000 records beyond the window on every end.  The universe is sized by long_grow,
    not by the growth: the members, a short span and 4 * 16,384 records are 65.6 thousand entries here, nearly all distinct.
    (More than 65,535 DISTINCT keys would need more than a thousand members and span records on top, which init_len = 700
    does not give: the members are some forty.)"""
    from sedef_amd import extz2
    rng = np.random.default_rng(31)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    n, p = 660_000, 330_000
    seq_q = bytes(rng.choice(acgt, n))
    seq_r = bytearray(bytes(rng.choice(acgt, n)))
    seq_r[p - 152_000:p + 1_500] = mutated(rng, seq_q[p - 152_000:p + 1_500], 0.07)
    seq_r = bytes(seq_r)
    eng.pool_upload(seq_q + seq_r)
    _, q = eng.pool_minimizers(eng.minim_ranges([(0, n)]))
    _, r = eng.pool_minimizers(eng.minim_ranges([(n, n)]))
    init_len = 700
    i = int(np.searchsorted(q["loc"], p))
    nm = members_end(q, i, init_len) - i
    windows = np.zeros(len(q), S.WINDOW)
    windows["n_members"], windows["query_size"] = 1, 1
    windows[i] = (len(set(R.keys_of(q[i:i + nm]))), nm, 0, 0, 0)
    first = np.zeros(len(q) + 1, np.int64)
    first[i + 1:] = 1
    intervals = np.array([(q["loc"][i], q["loc"][i] + 1)], S.INTERVAL)
    limit = np.maximum(1, np.arange(70_000) // 18).astype(np.int32)
    code, rolls = extz2.search_roll_host(q, windows, first, intervals, r, n, init_len, limit)
    assert code == 0 and rolls["jaccard"][0] >= 0 and rolls["flags"][0] == 0
    args = (q, windows, first, intervals, rolls, None, r, n, n, init_len, limit)
    params = dict(max_sd_size=330_000)
    want = host(args, params)
    g = grown(args, want, 0)
    assert want["flags"][0] == E.WIDE and 8192 < min(g) and max(g) <= LONG_MAX, g
    # the universe the kernel sorts: its distinct keys (a status-2 reference record stands as a member's key)
    G = LONG_MAX
    lo = int(np.searchsorted(r["loc"], intervals["start"][0]))
    uq = q[max(0, i - G):min(len(q), i + nm + G)]
    ur = r[max(0, min(int(rolls["winnow_start"][0]) - G, lo)):min(len(r), int(rolls["winnow_end"][0]) + G)]
    ur = ur[ur["status"] != 2]
    keys = np.concatenate([uq["status"].astype(np.int64) << 32 | uq["hash"], ur["status"].astype(np.int64) << 32 | ur["hash"]])
    assert len(keys) > 65_535 and len(np.unique(keys)) > 60_000
    u = Uploaded(eng, args, params)
    u.short()
    assert u.hits()[0].tolist() == ZERO_WIDE
    u.long(G)
    same_hits(u.hits(), want)
    assert u.left() == 0


def test_slots_beyond_sixteen_bits(eng):
    """Hand-built: every record of either side has a hash of its own but for the five members, which both sides share and which
    are the smallest keys, so that I stays 5 under a limit table of ones and every step is kept; the length stop ends the walk
    some 9,000 records out.  The universe at long_grow = 16,384 is 2 x (5 + 2 x 16,384) entries with 65,541 distinct keys: the
    boundary moves among dense slots that do not fit sixteen bits."""
    n, mid = 2 * LONG_MAX + 45, LONG_MAX + 16
    rng = np.random.default_rng(41)
    hashes = rng.permutation(np.arange(1 << 10, (1 << 10) + 2 * n))
    q = S.records(np.stack([hashes[:n], 2 * np.arange(n), np.zeros(n, np.int64)], 1))
    r = S.records(np.stack([hashes[n:], 2 * np.arange(n), np.zeros(n, np.int64)], 1))
    q["hash"][mid:mid + 5] = r["hash"][mid:mid + 5] = np.arange(1, 6)
    windows = np.zeros(n, S.WINDOW)
    windows["n_members"], windows["query_size"] = 1, 1
    windows[mid] = (5, 5, 0, 0, 0)
    first = np.zeros(n + 1, np.int64)
    first[mid + 1:] = 1
    intervals = np.array([(2 * mid, 2 * mid + 1)], S.INTERVAL)
    limit = np.ones(n + 2, np.int32)
    rolls = R.search_roll(q, windows, first, intervals, r, 2 * n, 10, limit)
    assert rolls["jaccard"][0] >= 0 and rolls["flags"][0] == 0
    args = (q, windows, first, intervals, rolls, None, r, 2 * n, 2 * n, 10, limit)
    params = dict(max_sd_size=36_000)
    want = host(args, params)
    g = grown(args, want, 0)
    assert want["flags"][0] == E.WIDE and 8192 < min(g) and max(g) <= LONG_MAX, g
    lo = int(np.searchsorted(r["loc"], intervals["start"][0]))
    uq = q[mid - LONG_MAX:mid + 5 + LONG_MAX]
    ur = r[min(int(rolls["winnow_start"][0]) - LONG_MAX, lo):int(rolls["winnow_end"][0]) + LONG_MAX]
    assert len(np.unique(np.concatenate([uq["hash"], ur["hash"]]))) > 65_535
    u = Uploaded(eng, args, params)
    u.short()
    assert u.hits()[0].tolist() == ZERO_WIDE
    u.long(LONG_MAX)
    same_hits(u.hits(), want)
    assert u.left() == 0


@pytest.fixture(scope="module")
def neighbours(records):
    """Four neighbouring windows of one duplication, every one grown by more than 1,792 records: their universes share keys."""
    at = (1900, 1901, 1902, 1903)
    args = identical_sequences(records, 3700, at)
    want = host(args, {})
    assert (want["flags"] == E.WIDE).all() and all(1792 < max(grown(args, want, t)) <= LONG for t in range(4))
    return args, want


@pytest.mark.parametrize("count", [3, 4])
def test_batch_seams(eng, neighbours, count):
    args, want = neighbours
    q, windows, first, intervals, rolls = args[:5]
    cut = (q, windows, np.minimum(first, count), intervals[:count], rolls[:count]) + args[5:]
    u = Uploaded(eng, cut, {})
    u.short()
    u.long(LONG, batch=2)
    same_hits(u.hits(), want[:count])
    assert u.left() == 0


def test_the_first_n_long_max_candidates_are_taken(eng, neighbours):
    args, want = neighbours
    u = Uploaded(eng, args, {})
    u.short()
    before = u.hits().copy()
    u.long(LONG, n_long_max=2, batch=2)
    got = u.hits()
    same_hits(got[:2], want[:2])
    assert got[2:].tobytes() == before[2:].tobytes() and got[2].tolist() == ZERO_WIDE and u.left() == 2
    u.long(LONG, n_long_max=1, batch=1)  # ... then the lowest of those that are left
    got = u.hits()
    same_hits(got[:3], want[:3])
    assert got[3].tolist() == ZERO_WIDE and u.left() == 1


def hand_built(n, mid, edit=None, n_limit=None):
    """Two lists of records, one every second base, with random hashes; `edit(q, r)` changes them in place.  The one interval
    of the window at `mid`."""
    rng = np.random.default_rng(3)
    q = S.records(np.stack([rng.integers(1, 1 << 20, n), 2 * np.arange(n), np.zeros(n, np.int64)], 1))
    r = q.copy()
    if edit:
        edit(q, r)
    windows = np.zeros(n, S.WINDOW)
    windows["n_members"], windows["query_size"] = 1, 1
    windows[mid] = (len(set(R.keys_of(q[mid:mid + 5]))), 5, 0, 0, 0)
    first = np.zeros(n + 1, np.int64)
    first[mid + 1:] = 1
    intervals = np.array([(2 * mid, 2 * mid + 1)], S.INTERVAL)
    limit = np.maximum(1, np.arange(n + 2 if n_limit is None else n_limit) // 2).astype(np.int32)
    rolls = R.search_roll(q, windows, first, intervals, r, 2 * n, 10, limit)
    assert rolls["jaccard"][0] >= 0
    return q, windows, first, intervals, rolls, None, r, 2 * n, 2 * n, 10, limit


def test_key_edges(eng):
    """roll_key all ones (status 3, hash 0x3FFFFFFF), roll_key 0, and status-2 records of either side inside the grown ranges."""
    def edit(q, r):
        for a in (q, r):
            for x in (40, 41, 1000, 1900, 1915, 2800, 3700):
                a[x] = (0x3FFFFFFF, a["loc"][x], 3, 0)
            for x in (7, 1001, 1899, 1920, 3001):
                a[x] = (0, a["loc"][x], 0, 0)
        q["status"][[300, 1500, 1908, 2500]] = 2
        r["status"][[301, 1500, 1700, 1913, 2400, 3500]] = 2
    n, mid = 2 * 1900 + 40, 1910
    args = hand_built(n, mid, edit)
    want = host(args, {})
    assert want["flags"][0] == E.WIDE and 1792 < max(grown(args, want, 0)) <= LONG and want["q_winnow_start"][0] == 0
    u = Uploaded(eng, args, {})
    u.short()
    u.long(LONG)
    same_hits(u.hits(), want)
    assert u.left() == 0


def test_growth_first_then_the_end_of_the_limit_table(eng):
    n, mid = 2 * E.MAX_GROW + 40, E.MAX_GROW + 10
    args = hand_built(n, mid, n_limit=2 * E.MAX_GROW + 12)
    want = host(args, {})
    assert want[0].tolist() == (0,) * 9 + (E.WIDE | E.NOLIMIT,)
    u = Uploaded(eng, args, {})
    u.short()
    assert u.hits()[0].tolist() == ZERO_WIDE
    u.long(LONG)
    same_hits(u.hits(), want)
    assert u.left() == 0
    # a table that ends before the growth: NOLIMIT alone from the short form, and the long form leaves it alone
    args = hand_built(n, mid, n_limit=200)
    u = Uploaded(eng, args, {})
    u.short()
    before = u.hits().copy()
    assert before[0].tolist() == (0,) * 9 + (E.NOLIMIT,)
    u.long(LONG)
    assert u.hits().tobytes() == before.tobytes() == host(args, {}).tobytes() and u.left() == 0


def test_every_other_record_stays_as_it_is(eng, records):
    """SKIPPED (the filter stopped it), not WIDE, WIDE because of the replay, and one candidate between them."""
    from sedef_amd import extz2
    at = (1000, 1001, 1800, 1801, 1802)
    count = members_end(records, 1000) + 1700
    q, windows, first, intervals, rolls, _, r, len_q, len_r, init_len, limit = identical_sequences(records, count, at)
    rolls = rolls.copy()
    rolls["flags"][3] |= 1  # SDF_ROLL_WIDE on a completed record: the replay does not fit a wavefront
    filt = np.zeros(len(rolls), extz2.FILTER_REC_DTYPE)
    filt["flags"][[1, 4]] = (2, 8)
    args = (q, windows, first, intervals, rolls, filt, r, len_q, len_r, init_len, limit)
    want = host(args, {})
    assert want["flags"].tolist() == [0, E.SKIPPED, E.WIDE, E.WIDE, E.SKIPPED] and (want["query_end"][[0, 2, 3]] != 0).all()
    u = Uploaded(eng, args, {})
    u.short()
    before = u.hits().copy()
    assert before[2].tolist() == ZERO_WIDE and before[3].tolist() == ZERO_WIDE
    u.long(LONG)
    got = u.hits()
    others = [0, 1, 3, 4]
    assert got[others].tobytes() == before[others].tobytes() and got[2].tobytes() == want[2].tobytes() and u.left() == 0
    # a smaller n_max: the records at and behind it are not looked at
    u = Uploaded(eng, args, {})
    u.short()
    u.long(LONG, n_max=2)
    assert u.hits().tobytes() == before.tobytes() and u.left() == 0


def test_chained_on_one_stream_to_the_second_filter(eng, two_growths):
    """extend -> extend_long -> hit tasks -> filter on the caller's stream, one synchronisation at the end."""
    from sedef_amd import extz2
    args, want = two_growths[0]
    len_q, len_r = args[7], args[8]
    pool = bytes(np.random.default_rng(8).choice(np.frombuffer(b"ACGTacgtN", np.uint8), len_q + len_r + 20))
    q_off, r_off = 5, len_q + 11
    eng.pool_upload(pool)
    eng.lib.sdf_pool_sync(eng.ctx)
    u = Uploaded(eng, args, {})
    cap = u.n + 3
    d_tasks = torch.zeros(cap * 32, dtype=torch.uint8, device="cuda")
    d_recs = torch.zeros(cap * 20, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    st = stream.cuda_stream
    u.short(stream=st)
    u.long(LONG, stream=st)
    eng.search_hit_tasks_device(u.d_hits.data_ptr(), cap, u.keep[2].data_ptr() + 8 * len(args[0]), len_q, len_r, q_off, False, r_off, False,
                                d_tasks.data_ptr(), stream=st)
    eng.search_filter_device(d_tasks.data_ptr(), cap, False, d_recs.data_ptr(), extz2.filter_params(), stream=st)
    stream.synchronize()
    same_hits(u.hits(), want)
    code, tasks = extz2.search_hit_tasks_host(want, len_q, len_r, q_off, False, r_off, False)
    assert code == 0 and (tasks["flags"] & 4 == 0).all()
    code, recs = extz2.search_filter_host(pool, tasks)
    assert code == 0
    got = np.frombuffer(d_recs.cpu().numpy().tobytes(), extz2.FILTER_REC_DTYPE)
    assert got[:u.n].tobytes() == recs.tobytes() and (got["flags"][u.n:] == 8).all() and (recs["q_up"] > 1000).all()


def test_combined_form_runs_the_long_form(eng, two_growths):
    from sedef_amd import extz2
    args, want = two_growths[0]
    before = eng.last_launches()
    code, got = eng.search_extend_raw(*args)
    assert code == 0, eng.lib.sdf_last_error(eng.ctx).decode()
    same_hits(got, want)
    assert eng.last_launches() - before == 1 + 3 + 6  # the short form, the selection, one batch of two
    # without a candidate: the short form's launch alone
    short = identical_sequences(args[0], 900, (400,))
    want = host(short, {})
    assert want["flags"].tolist() == [0]
    before = eng.last_launches()
    code, got = eng.search_extend_raw(*short)
    assert code == 0 and eng.last_launches() - before == 1
    same_hits(got, want)


def test_refusals_and_empties(eng, two_growths):
    from sedef_amd import extz2
    args, want = two_growths[0]
    u = Uploaded(eng, args, {})
    u.short()
    start = u.hits().copy()
    before = eng.last_launches()

    def refused(code, **kw):
        assert u.long(**dict(dict(long_grow=LONG, check=False), **kw)) == code, kw
        assert eng.last_launches() == before and eng.lib.sdf_last_error(eng.ctx) != b""
    refused(SDF_ERR_INVALID, long_grow=extz2.EXTEND_MAX_GROW)
    refused(SDF_ERR_INVALID, long_grow=extz2.EXTEND_LONG_MAX_GROW + 1)
    refused(SDF_ERR_INVALID, long_grow=-5)
    for bad in (dict(max_error=0.1), dict(max_error=float("nan"))):  # as sdf_search_extend_device refuses
        good, u.params = u.params, extz2.extend_params(**bad)
        refused(SDF_ERR_INVALID)
        u.params = good
    good, u.params = u.params, extz2.extend_params(reserved=(0, 1))
    refused(SDF_ERR_UNSUPPORTED)
    u.params = good
    import ctypes as C
    P = C.byref(u.params)
    call = lambda head, tail, hits: eng.lib.sdf_search_extend_long_device(eng.ctx, *head, u.n, *tail, P, LONG, 5, 0, hits, None, None)  # noqa: E731
    assert call(u.head, u.tail, None) == SDF_ERR_INVALID  # no d_hits with work to do
    assert call((None,) + u.head[1:], u.tail, u.d_hits.data_ptr()) == SDF_ERR_INVALID
    assert call(u.head, u.tail[:4] + (0,) + u.tail[5:], u.d_hits.data_ptr()) == SDF_ERR_INVALID  # init_len
    assert call(u.head, u.tail[:2] + (1 << 31,) + u.tail[3:], u.d_hits.data_ptr()) == SDF_ERR_UNSUPPORTED  # len_q
    # a workspace beyond the context's budget: refused before the first launch
    import sedef_amd
    small = sedef_amd.Extz2Engine(0, workspace_bytes=1 << 16)
    try:
        v = Uploaded(small, args, {})
        v.short()
        launches = small.last_launches()
        assert v.long(LONG, check=False) == SDF_ERR_NOMEM and small.last_launches() == launches
        same_hits(v.hits(), start)
    finally:
        small.close()
    assert eng.last_launches() == before
    # nothing to do: no launch, nothing written
    assert u.long(LONG, n_long_max=0) == 0 and u.long(LONG, n_max=0) == 0 and eng.last_launches() == before
    assert call((u.head[0], 0) + u.head[2:], u.tail, u.d_hits.data_ptr()) == 0 and eng.last_launches() == before
    assert u.left() == 77 and u.hits().tobytes() == start.tobytes()
    # ... and no candidate: d_left is 0, no record changes
    short = identical_sequences(args[0], 900, (400,))
    v = Uploaded(eng, short, {})
    v.short()
    only = v.hits().copy()
    assert v.long(LONG) == 0 and v.left() == 0 and v.hits().tobytes() == only.tobytes() == host(short, {}).tobytes()
    assert v.long(LONG, left=False) == 0
