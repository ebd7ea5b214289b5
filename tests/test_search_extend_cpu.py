"""CPU: the search extension -- every rolled interval grown to its hit (include/sedef_hip.h: sdf_search_extend) -- pinned on
the reference (tests/golden/search_extend_kat.json.gz, written by tests/golden/make_golden_search_extend.py from the
reference's own SlidingMap and Index):
  * tests/extend_model.py, the header's rules with a dict and a sorted list, gives the fixture's records;
  * sdf_search_extend_host, the same rules in C++ behind the C ABI (no context, no GPU; a map), gives the fixture's records
    and the model's on random inputs, and keeps the refusals of the header;
  * sdf_search_hit_tasks_host gives the tasks a few lines of Python give."""
import gzip
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import extend_model as E  # noqa: E402
import roll_model as R  # noqa: E402
from test_search_roll_cpu import case_inputs, random_inputs  # noqa: E402

SDF_ERR_UNSUPPORTED, SDF_ERR_INVALID = -3, -4


def load_fixture():
    with gzip.open(os.path.join(ROOT, "tests", "golden", "search_extend_kat.json.gz"), "rb") as f:
        return json.loads(f.read().decode())


@pytest.fixture(scope="module")
def fixture():
    return load_fixture()


def case_params(c):
    return dict(max_error=c["max_error"], max_edit_error=c["max_edit_error"], max_sd_size=c["max_sd_size"], same_genome=c["same_genome"])


def case_extend_inputs(c):
    """A fixture case as the extension takes it: (q, windows, first, intervals, rolls, None, r, len_q, len_r, init_len, limit)
    and its parameters; the rolls are the fixture's."""
    q, windows, first, intervals, r, len_r, init_len, limit = case_inputs(c)
    rows = [tuple(t[2:7]) + (0,) for w in c["windows"] for t in w[2]]
    rolls = np.array(rows, R.ROLL) if rows else np.zeros(0, R.ROLL)
    return (q, windows, first, intervals, rolls, None, r, len(c["q"]), len_r, init_len, limit), case_params(c)


def case_expected(c):
    rows = [tuple(t[8:17]) + (t[7],) for w in c["windows"] for t in w[2]]
    return np.array(rows, E.HIT) if rows else np.zeros(0, E.HIT)


@pytest.fixture(scope="module")
def inputs(fixture):
    """Every case's arrays, computed once."""
    return [case_extend_inputs(c) for c in fixture["cases"]]


def model(args, params, **kw):
    q, windows, first, intervals, rolls, filt, r, len_q, len_r, init_len, limit = args
    return E.search_extend(q, windows, first, intervals, r, len_r, init_len, limit, rolls, len_q, filt, params, **kw)


def host(args, params):
    from sedef_amd import extz2
    return extz2.search_extend_host(*args, extz2.extend_params(**params))


def same_hits(got, want, what=""):
    assert got.tobytes() == want.tobytes(), (what, [(int(t), got[t], want[t]) for t in np.flatnonzero(got != want)[:5]])


def random_extend_inputs(rng, **kw):
    """random_inputs of the roll's test with the roll model's records, a query length and a filter array that stops a few."""
    q, windows, first, intervals, r, len_r, init_len, limit = random_inputs(rng, **kw)
    limit = rng.integers(0, int(rng.choice([5, 9, 14])), 70).astype(np.int32)
    rolls = R.search_roll(q, windows, first, intervals, r, len_r, init_len, limit)
    filt = np.zeros(len(rolls), [("q_up", "<i4"), ("r_up", "<i4"), ("dist", "<i4"), ("minqg", "<i4"), ("flags", "<u4")])
    filt["flags"] = rng.choice([0, 0, 0, 0, 4, 1, 2, 8], len(rolls))
    return q, windows, first, intervals, rolls, filt, r, int(q["loc"][-1]) + 4, len_r, init_len, limit


def test_fixture_has_every_quirk(fixture):
    cases = fixture["cases"]
    for name in ("undos", "false_add_undos", "stop_len", "stop_ratio", "stop_overlap", "at_end"):
        assert sum(c["counters"][name] for c in cases) > 0, name
    rows = [t for c in cases for w in c["windows"] for t in w[2]]
    hits = [t for t in rows if t[7] == 0]
    assert len(hits) >= 2000 and 5 * sum(t[16] - t[15] > t[5] - t[4] for t in hits) >= len(hits)
    assert any(t[7] == E.NOLIMIT for t in rows) and any(t[7] == E.SKIPPED for t in rows)
    k12 = [c for c in cases if c["k"] == 12 and c["w"] == 16 and c["init_len"] == 700]
    assert len(k12) >= 3 and any(c["same_genome"] for c in k12) and any(c["r_rc"] for c in k12)


def test_model_gives_the_fixture(fixture, inputs):
    seen = {}
    for c, (args, params) in zip(fixture["cases"], inputs):
        same_hits(model(args, params, seen=seen), case_expected(c), c["name"])
    assert seen.get("guards", 0) == 0  # (no committed case reaches what the reference leaves undefined)
    for name in ("undos", "false_add_undos", "stop_len", "stop_ratio", "stop_overlap", "at_end"):
        assert seen[name] == sum(c["counters"][name] for c in fixture["cases"]), name


def test_a_restoring_undo_gives_other_hits(fixture, inputs, monkeypatch):
    """The point of the literal undo: with remove_from_query that leaves alone what its do never set, hits differ."""
    moved = 0
    plain = E.Sliding.add_to_query

    def add_to_query(self, key):
        ok = plain(self, key)
        self.skip = getattr(self, "skip", set())
        (self.skip.discard if ok else self.skip.add)(key)
        return ok

    def remove_from_query(self, key, undo=E.Sliding.remove_from_query):
        if key not in getattr(self, "skip", ()):
            undo(self, key)
    monkeypatch.setattr(E.Sliding, "add_to_query", add_to_query)
    monkeypatch.setattr(E.Sliding, "remove_from_query", remove_from_query)
    for c, (args, params) in zip(fixture["cases"], inputs):
        if c["counters"]["false_add_undos"]:
            moved += int((model(args, params) != case_expected(c)).sum())
    assert moved > 0


def test_host_form_gives_the_fixture(fixture, inputs):
    for c, (args, params) in zip(fixture["cases"], inputs):
        code, got = host(args, params)
        assert code == 0, c["name"]
        same_hits(got, case_expected(c), c["name"])


def test_host_form_equals_the_model_on_random_inputs():
    rng = np.random.default_rng(12)
    seen, n_hits = {}, 0
    for it in range(40):
        args = random_extend_inputs(rng, init_len=int(rng.choice([1, 6, 25, 90])), dup_locs=bool(it % 2), hashes=int(rng.choice([5, 9, 40])))
        params = dict(max_error=float(rng.choice([0.3, 0.25])), max_edit_error=float(rng.choice([0.15, 0.05])),
                      max_sd_size=int(rng.choice([1 << 20, 300])), same_genome=it % 3 == 0)
        if it % 4 == 3:
            args = args[:5] + (None,) + args[6:]
        code, got = host(args, params)
        assert code == 0
        want = model(args, params, seen=seen)
        same_hits(got, want, it)
        n_hits += int((want["flags"] == 0).sum())
    assert n_hits > 300 and seen["undos"] > 0 and seen["false_add_undos"] > 0, seen


def wide_growth_inputs():
    """Two identical lists of records, one every second base, with random hashes: the extension of the window in the middle
    runs to both ends, past the growth cap, and query_size grows with every step.  Returns (args, the number of records)."""
    n = 2 * E.MAX_GROW + 40
    rng = np.random.default_rng(3)
    import search_model as S
    q = S.records(np.stack([rng.integers(0, 1 << 20, n), 2 * np.arange(n), np.zeros(n, np.int64)], 1))
    windows = np.zeros(n, S.WINDOW)
    windows["n_members"], windows["query_size"] = 1, 1
    mid = E.MAX_GROW + 10
    windows[mid] = (5, 5, 0, 0, 0)
    first = np.zeros(n + 1, np.int64)
    first[mid + 1:] = 1
    intervals = np.array([(2 * mid, 2 * mid + 1)], S.INTERVAL)
    limit = np.maximum(1, np.arange(n + 2) // 2).astype(np.int32)
    rolls = R.search_roll(q, windows, first, intervals, q, 2 * n, 10, limit)
    assert rolls["jaccard"][0] >= 0
    return (q, windows, first, intervals, rolls, None, q, 2 * n, 2 * n, 10, limit), n


def test_host_form_flags_wide_growth_and_completes_it():
    args, n = wide_growth_inputs()
    limit = args[-1]
    code, got = host(args, {})
    assert code == 0 and got["flags"].tolist() == [E.WIDE] and got["q_winnow_start"][0] == 0 and got["q_winnow_end"][0] == n
    same_hits(got, model(args, {}))
    assert model(args, {}, device=True)[0].tolist() == (0,) * 9 + (E.WIDE,)
    # the growth comes first, then an add needs the table beyond its end: the device form ends at the growth and says WIDE,
    # the host form walks on and answers WIDE | NOLIMIT -- the flag the device set is kept
    short = limit[:2 * E.MAX_GROW + 12]
    assert len(short) < n
    args = args[:-1] + (short,)
    code, got = host(args, {})
    assert code == 0 and got[0].tolist() == (0,) * 9 + (E.WIDE | E.NOLIMIT,)
    same_hits(got, model(args, {}))
    assert model(args, {}, device=True)[0].tolist() == (0,) * 9 + (E.WIDE,)
    # ... and a table that ends before the growth does: NOLIMIT alone, in every form
    args = args[:-1] + (limit[:200],)
    code, got = host(args, {})
    assert code == 0 and got[0].tolist() == (0,) * 9 + (E.NOLIMIT,)
    same_hits(got, model(args, {}))
    same_hits(got, model(args, {}, device=True))


def test_hit_tasks_host_form():
    from sedef_amd import extz2
    rng = np.random.default_rng(4)
    hits = np.zeros(300, E.HIT)
    for name in ("query_start", "ref_start"):
        hits[name] = rng.integers(-2, 500, len(hits))
    hits["query_end"] = hits["query_start"] + rng.integers(-1, 300, len(hits))
    hits["ref_end"] = hits["ref_start"] + rng.integers(-1, 300, len(hits))
    hits["flags"] = rng.choice([0, 0, 0, 1, 2, 4], len(hits))
    hits["query_end"][hits["flags"] == 2] *= rng.integers(0, 2, int((hits["flags"] == 2).sum()))
    n_live = 0
    for q_rc, r_rc in ((0, 0), (1, 0), (0, 1), (1, 1)):
        code, got = extz2.search_hit_tasks_host(hits, 700, 650, 1000, q_rc, 5000, r_rc)
        assert code == 0
        want = np.array([E.hit_task(h, 700, 650, 1000, q_rc, 5000, r_rc) for h in hits], extz2.FILTER_TASK_DTYPE)
        assert got.tobytes() == want.tobytes()
        n_live += int((want["flags"] & 4 == 0).sum())
    assert 200 < n_live < 1100
    assert extz2.search_hit_tasks_host(hits, -1, 650, 0, 0, 0, 0)[0] == SDF_ERR_INVALID
    assert extz2.search_hit_tasks_host(hits, 700, 650, 0, 0, -1, 0)[0] == SDF_ERR_INVALID
    assert extz2.search_hit_tasks_host(hits, 1 << 31, 650, 0, 0, 0, 0)[0] == SDF_ERR_UNSUPPORTED
    assert extz2.search_hit_tasks_host(hits[:0], 700, 650, 0, 0, 0, 0)[0] == 0


def test_refusals():
    from sedef_amd import extz2
    rng = np.random.default_rng(2)
    args = random_extend_inputs(rng)
    names = ("q", "windows", "first", "intervals", "rolls", "filt", "r", "len_q", "len_r", "init_len", "limit")
    good = dict(zip(names, args))

    def code(params=None, **change):
        return extz2.search_extend_host(*dict(good, **change).values(), extz2.extend_params(**(params or {})))[0]
    assert code() == 0
    assert code(init_len=0) == SDF_ERR_INVALID and code(init_len=(1 << 30) + 1) == SDF_ERR_UNSUPPORTED
    assert code(len_r=-1) == SDF_ERR_INVALID and code(len_r=1 << 31) == SDF_ERR_UNSUPPORTED
    assert code(len_q=-1) == SDF_ERR_INVALID and code(len_q=1 << 31) == SDF_ERR_UNSUPPORTED
    assert code(dict(max_error=float("nan"))) == SDF_ERR_INVALID and code(dict(max_edit_error=float("inf"))) == SDF_ERR_INVALID
    assert code(dict(max_error=0.15, max_edit_error=0.15)) == SDF_ERR_INVALID and code(dict(max_error=0.1)) == SDF_ERR_INVALID
    assert code(dict(reserved=(0, 1))) == SDF_ERR_UNSUPPORTED and code(dict(reserved=(1, 0))) == SDF_ERR_UNSUPPORTED
    first, intervals = good["first"], good["intervals"]
    t = int(np.flatnonzero(np.diff(first))[0])
    bad = intervals.copy()
    bad[first[t]] = (5, 4)
    assert code(intervals=bad) == SDF_ERR_INVALID
    w = good["windows"].copy()
    w["query_size"][t] = len(good["limit"])
    assert code(windows=w) == SDF_ERR_INVALID
    # null arrays; nq == 0 and no interval at all are fine
    fn = extz2.load_library().sdf_search_extend_host
    import ctypes as C
    P = extz2.extend_params()
    q, windows, f64, r, limit = good["q"], good["windows"], first.astype(np.uint64), good["r"], good["limit"]
    rolls = np.ascontiguousarray(good["rolls"], extz2.SEARCH_ROLL_DTYPE)
    out = np.zeros(len(intervals), extz2.SEARCH_HIT_DTYPE)
    ok = [q.ctypes.data, len(q), windows.ctypes.data, f64.ctypes.data, intervals.ctypes.data, rolls.ctypes.data, None, r.ctypes.data,
          len(r), good["len_q"], good["len_r"], good["init_len"], limit.ctypes.data, len(limit), C.byref(P), out.ctypes.data]
    assert fn(*ok) == 0
    for at in (0, 2, 3, 4, 5, 7, 12, 14, 15):
        call = list(ok)
        call[at] = None
        assert fn(*call) == SDF_ERR_INVALID, at
    assert fn(None, 0, None, None, None, None, None, None, 0, 100, 100, 10, None, 0, None, None) == 0
    none = np.zeros(len(q) + 1, np.uint64)
    assert fn(q.ctypes.data, len(q), windows.ctypes.data, none.ctypes.data, None, None, None, None, 0, 100, 100, 10, None, 0, None, None) == 0
