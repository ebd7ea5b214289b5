"""CPU: the search roll -- every reference interval rolled to its best initial match (include/sedef_hip.h: sdf_search_roll) --
pinned on the reference (tests/golden/search_roll_kat.json.gz, written by tests/golden/make_golden_search_roll.py from the
reference's own SlidingMap and Index::find_minimizers):
  * tests/roll_model.py, the header's rules with a dict and a sorted list, one base a step, gives the fixture's records;
  * sdf_search_roll_host, the same rules in C++ behind the C ABI (no context, no GPU; a map, from event to event), gives the
    fixture's records and the model's on random inputs, and keeps the refusals of the header."""
import gzip
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import minim_model as M  # noqa: E402
import roll_model as R  # noqa: E402
import search_model as S  # noqa: E402
from test_search_windows_cpu import case_args, case_sequences  # noqa: E402

SDF_ERR_UNSUPPORTED, SDF_ERR_INVALID = -3, -4


def load_fixture():
    with gzip.open(os.path.join(ROOT, "tests", "golden", "search_roll_kat.json.gz"), "rb") as f:
        return json.loads(f.read().decode())


@pytest.fixture(scope="module")
def fixture():
    return load_fixture()


def case_inputs(c):
    """A fixture case as the roll takes it: (q, windows, first, intervals, r in loc order, len_r, init_len, limit), the
    front half by tests/search_model.py -- whose intervals must be the fixture's."""
    qs, rs = case_sequences(c)
    q = S.records(M.get_minimizers(qs, c["k"], c["w"], bool(c["sl"])))
    r = q if c["same"] else S.records(M.get_minimizers(rs, c["k"], c["w"], bool(c["sl"])))
    first, windows, intervals = S.search_windows(q, S.index_order(r), **case_args(c))
    want = [t[:2] for w in c["windows"] for t in w[2]]
    assert np.array_equal(first, np.cumsum([0] + [len(w[2]) for w in c["windows"]])), c["name"]
    assert np.stack([intervals["start"], intervals["end"]], 1).tolist() == want, c["name"]
    assert windows["query_size"].tolist() == [w[0] for w in c["windows"]], c["name"]
    return q, windows, first, intervals, r, len(rs), c["init_len"], np.array(c["limit"], np.int32)


def case_expected(c):
    """The fixture's records of a case (no interval of the fixture is WIDE)."""
    rows = [tuple(t[2:]) + (0,) for w in c["windows"] for t in w[2]]
    return np.array(rows, R.ROLL) if rows else np.zeros(0, R.ROLL)


@pytest.fixture(scope="module")
def inputs(fixture):
    """Every case's arrays, computed once."""
    return [case_inputs(c) for c in fixture["cases"]]


def host(*args):
    from sedef_amd import extz2
    return extz2.search_roll_host(*args)


def same_rolls(got, want, what=""):
    assert got.tobytes() == want.tobytes(), (what, [(int(t), got[t], want[t]) for t in np.flatnonzero(got != want)[:5]])


def random_inputs(rng, nq=60, nr=160, hashes=9, len_r=400, init_len=25, dup_locs=True):
    """Arrays the entry points accept, not the output of a front half: keys from a small alphabet, every status, windows of 1
    to 12 members, 0 to 3 intervals a window anywhere on the reference, some of them reaching len_r."""
    def minimizers(n, top):
        locs = np.sort(rng.choice(top, n, replace=dup_locs))
        return S.records(np.stack([rng.integers(0, hashes, n), locs, rng.choice([0, 0, 0, 1, 1, 2], n)], 1))
    q, r = minimizers(nq, 3000), minimizers(nr, len_r - 3)
    windows = np.zeros(nq, S.WINDOW)
    rows, first = [], [0]
    limit = rng.integers(0, 5, 16).astype(np.int32)
    for i in range(nq):
        nm = int(rng.integers(1, min(12, nq - i) + 1))
        windows[i] = (int(rng.integers(0, 16)), nm, 0, 0, 0)
        for _ in range(int(rng.choice([0, 0, 1, 2, 3]))):
            start = int(rng.integers(0, len_r + 5))
            rows.append((start, start + int(rng.choice([0, 1, 7, 40, 120]))))
        first.append(len(rows))
    intervals = np.array(rows, np.int64).reshape(-1, 2).astype("<i4").view(S.INTERVAL).reshape(-1)
    return q, windows, np.array(first, np.int64), intervals, r, len_r, init_len, limit


def test_fixture_counters_are_above_zero(fixture):
    cases = fixture["cases"]
    for name in R.COUNTERS:
        assert sum(c["counters"][name] for c in cases) > 0, name
    k12 = [c for c in cases if c["k"] == 12 and c["w"] == 16 and c["init_len"] == 700]
    assert len(k12) >= 3 and any(c["same_genome"] for c in k12) and any(c["r_rc"] for c in k12)
    assert sum(len(w[2]) for c in cases for w in c["windows"]) >= 2000


def test_model_gives_the_fixture(fixture, inputs):
    seen = {}
    for c, args in zip(fixture["cases"], inputs):
        same_rolls(R.search_roll(*args, seen=seen), case_expected(c), c["name"])
    assert seen.get("negative", 0) and seen.get("dup_removes", 0) > 0 and seen.get("adds_on_boundary", 0) > 0


def test_host_form_gives_the_fixture(fixture, inputs):
    for c, args in zip(fixture["cases"], inputs):
        code, got = host(*args)
        assert code == 0, c["name"]
        same_rolls(got, case_expected(c), c["name"])


def test_host_form_equals_the_model_on_random_inputs():
    rng = np.random.default_rng(11)
    moved = 0
    for it in range(30):
        args = random_inputs(rng, init_len=int(rng.choice([1, 6, 25, 90])), dup_locs=bool(it % 2))
        code, got = host(*args)
        assert code == 0
        want = R.search_roll(*args)
        same_rolls(got, want, it)
        moved += int((want["ref_start"] != args[3]["start"]).sum())
    assert moved > 100


def test_host_form_flags_wide_intervals_and_completes_them():
    q = S.records([(j % 7, j, 0) for j in range(1100)])
    r = S.records([(j % 5, 2 * j, 0) for j in range(2000)])
    windows = np.zeros(len(q), S.WINDOW)
    windows["n_members"], windows["query_size"] = 1, 1
    windows[0] = (7, 1025, 0, 0, 0)
    windows[1] = (7, 1024, 0, 0, 0)
    first = np.zeros(len(q) + 1, np.int64)
    first[1], first[2:] = 1, 2
    intervals = np.array([(10, 60), (10, 60)], S.INTERVAL)
    args = (q, windows, first, intervals, r, 4000, 50, np.arange(9, dtype=np.int32))
    code, got = host(*args)
    assert code == 0 and got["flags"].tolist() == [R.WIDE, 0]
    same_rolls(got, R.search_roll(*args))
    assert R.search_roll(*args, device=True)[0].tolist() == (0, 0, 0, 0, 0, R.WIDE)


def test_refusals():
    rng = np.random.default_rng(2)
    q, windows, first, intervals, r, len_r, init_len, limit = random_inputs(rng)
    good = dict(q=q, windows=windows, first=first, intervals=intervals, r=r, len_r=len_r, init_len=init_len, limit=limit)

    def code(**change):
        return host(*dict(good, **change).values())[0]
    assert code() == 0
    assert code(init_len=0) == SDF_ERR_INVALID and code(init_len=(1 << 30) + 1) == SDF_ERR_UNSUPPORTED
    assert code(len_r=-1) == SDF_ERR_INVALID and code(len_r=1 << 31) == SDF_ERR_UNSUPPORTED
    assert code(r=r[:0]) == SDF_ERR_INVALID  # intervals without a reference record
    t = int(np.flatnonzero(np.diff(first))[0])  # a window with an interval
    bad = intervals.copy()
    bad[first[t]] = (5, 4)
    assert code(intervals=bad) == SDF_ERR_INVALID
    bad[first[t]] = (-1, 4)
    assert code(intervals=bad) == SDF_ERR_INVALID
    for field, value in (("query_size", len(limit)), ("query_size", -1), ("n_members", 0), ("n_members", len(q) - t + 1)):
        w = windows.copy()
        w[field][t] = value
        assert code(windows=w) == SDF_ERR_INVALID, (field, value)
    idle = int(np.flatnonzero(np.diff(first) == 0)[0])  # ... a window without one is not looked at
    w = windows.copy()
    w["query_size"][idle] = len(limit)
    assert code(windows=w) == 0
    down = first.copy()
    down[t] = first[t + 1] + 1  # (first[0] != 0, or first[t + 1] < first[t])
    assert code(first=down) == SDF_ERR_INVALID
    # null arrays; nq == 0 and no interval at all are fine
    from sedef_amd import extz2
    fn = extz2.load_library().sdf_search_roll_host
    out = np.zeros(len(intervals), extz2.SEARCH_ROLL_DTYPE)
    f64 = first.astype(np.uint64)
    ok = [q.ctypes.data, len(q), windows.ctypes.data, f64.ctypes.data, intervals.ctypes.data, r.ctypes.data, len(r), len_r, init_len,
          limit.ctypes.data, len(limit), out.ctypes.data]
    assert fn(*ok) == 0
    for at in (0, 2, 3, 4, 5, 9, 11):
        args = list(ok)
        args[at] = None
        assert fn(*args) == SDF_ERR_INVALID, at
    assert fn(None, 0, None, None, None, None, 0, 100, 10, None, 0, None) == 0
    none = np.zeros(len(q) + 1, np.uint64)
    assert fn(q.ctypes.data, len(q), windows.ctypes.data, none.ctypes.data, None, None, 0, 100, 10, None, 0, None) == 0
