"""CPU: the search filter -- uppercase and q-gram verdicts per pair of pool ranges (include/sedef_hip.h: sdf_search_filter) --
pinned on the reference (tests/golden/search_filter_kat.json.gz, written by tests/golden/make_golden_search_filter.py from the
reference's own filter()):
  * tests/filter_model.py, the header's rules in numpy, gives the fixture's records and its minqg sweep;
  * sdf_search_filter_host and sdf_search_filter_tasks_host, the same in C++ behind the C ABI (no context, no GPU), give the
    fixture's records and tasks, and keep the refusals of the header without writing anything."""
import gzip
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import filter_model as F  # noqa: E402

SDF_ERR_UNSUPPORTED, SDF_ERR_INVALID = -3, -4
COUNTERS = ("passes", "upper_fail", "qgram_fail", "short", "rc_sides", "short_sides", "final_differs")


def load_fixture():
    with gzip.open(os.path.join(ROOT, "tests", "golden", "search_filter_kat.json.gz"), "rb") as f:
        return json.loads(f.read().decode())


@pytest.fixture(scope="module")
def fixture():
    return load_fixture()


def case_tasks(c):
    rows = [tuple(t) + (0,) for t in c["tasks"]]
    return np.array(rows, F.TASK) if rows else np.zeros(0, F.TASK)


def params_of(P):
    from sedef_amd import extz2
    return extz2.filter_params(**P)


def host(pool, tasks, P, **kw):
    from sedef_amd import extz2
    return extz2.search_filter_host(pool, tasks, params_of(P), **kw)


def same_as_fixture(got, c, what=""):
    """Every record the reference printed whole: the same 20 bytes; a verdict-only one: q_up, r_up and the two verdict bits."""
    assert len(got) == len(c["records"])
    for t, (g, w) in enumerate(zip(got.tolist(), c["records"])):
        if w[2] is None:
            assert (g[0], g[1], g[4] & 3) == (w[0], w[1], w[4]), (what, c["name"], t, g, w)
        else:
            assert list(g) == w, (what, c["name"], t, g, w)


def test_fixture_counters_are_above_zero(fixture):
    cases = fixture["cases"]
    for name in COUNTERS:
        assert sum(c["counters"][name] for c in cases) > 0, name
    pairs = sum(len(c["tasks"]) for c in cases)
    assert pairs >= 1500 and 10 * sum(c["counters"]["verdict_only"] for c in cases) <= pairs
    assert {c["allow_extend"] for c in cases if "roll_case" in c} == {0, 1}
    assert all(len(s["minqg"]) == 2200 and s["minqg"][-1][0] == 1 << 20 for s in fixture["sweep"]) and len(fixture["sweep"]) == 3


def test_model_gives_the_fixture(fixture):
    for c in fixture["cases"]:
        same_as_fixture(F.filter_pairs(c["pool"].encode(), case_tasks(c), **c["params"]), c, "model")


def test_host_form_gives_the_fixture(fixture):
    for c in fixture["cases"]:
        code, got = host(c["pool"].encode(), case_tasks(c), c["params"])
        assert code == 0
        same_as_fixture(got, c, "host form")
        # ... and the model's bytes also where the reference printed the verdict alone
        assert got.tobytes() == F.filter_pairs(c["pool"].encode(), case_tasks(c), **c["params"]).tobytes(), c["name"]


def test_minqg_sweep(fixture):
    """minqg of every l of the sweep by the model and by the host form (one side of l characters against an empty one: dist 0),
    equal to what the reference printed -- it prints nothing exactly where minqg <= 0."""
    pool = b"a" * (1 << 20)
    for s in fixture["sweep"]:
        P = s["params"]
        want = [F.minqg(l, **P) for l, _ in s["minqg"]]
        assert sum(m is not None for _, m in s["minqg"]) > 1500
        for (l, m), w in zip(s["minqg"], want):
            assert (m == w and m > 0) if m is not None else w <= 0, (P, l, m, w)
        tasks = np.zeros(len(want), F.TASK)
        tasks["q_len"] = [l for l, _ in s["minqg"]]
        code, got = host(pool, tasks, dict(P, min_uppercase=0))
        assert code == 0 and got["minqg"].tolist() == want and not got["dist"].any()
        assert ((got["flags"] & F.QGRAM_FAIL) != 0).tolist() == [w > 0 for w in want]
        assert ((got["flags"] & F.SHORT) != 0).tolist() == [w < 10 for w in want]


def roll_arrays(c):
    import test_search_roll_cpu as T
    rc = next(x for x in T.load_fixture()["cases"] if x["name"] == c["roll_case"])
    return rc, T.case_inputs(rc), T.case_expected(rc)


def test_task_builder_on_the_roll_cases(fixture):
    from sedef_amd import extz2
    differs = 0
    cases = [c for c in fixture["cases"] if "roll_case" in c]
    assert len(cases) >= 4
    for c in cases:
        rc, (q, windows, first, intervals, r, len_r, init_len, limit), rolls = roll_arrays(c)
        args = (q, windows, first, intervals, rolls, len(rc["q"]), len_r, init_len, c["q_off"], 0, c["r_off"], rc["r_rc"], c["allow_extend"])
        want = case_tasks(c)
        assert F.filter_tasks(*args).tobytes() == want.tobytes(), c["name"]
        code, got = extz2.search_filter_tasks_host(*args)
        assert code == 0 and got.tobytes() == want.tobytes(), c["name"]
        assert ((rolls["jaccard"] < 0) == ((got["flags"] & F.SKIP) != 0)).all()
        if c["allow_extend"]:  # the final position, not the best one
            code, best = extz2.search_filter_tasks_host(*args[:-1], 0)
            differs += int((best["r_off"] != got["r_off"]).sum())
            assert int((best["r_off"] != got["r_off"]).sum()) == c["counters"]["final_differs"]
    assert differs > 100


def test_task_builder_skips_and_strands():
    import search_model as S
    import roll_model as R
    from sedef_amd import extz2
    q = S.records([(5, 10, 0), (6, 40, 0), (7, 90, 0)])
    windows = np.array([(1, 1, 0, 0, 0), (1, 1, 0, 0, S.NOLIMIT), (1, 1, 0, 0, 0)], S.WINDOW)
    first = np.array([0, 4, 5, 7], np.int64)
    intervals = np.array([(100, 130), (100, 130), (100, 130), (100, 130), (0, 9), (280, 300), (250, 400)], S.INTERVAL)
    rolls = np.array([(110, 130, 0, 0, 3, 0), (110, 130, 0, 0, -1, 0), (0, 0, 0, 0, 0, R.WIDE), (110, 130, 0, 0, 2, R.WIDE),
                      (0, 20, 0, 0, 1, 0), (280, 300, 0, 0, 0, 0), (260, 280, 0, 0, 5, 2)], R.ROLL)
    for q_rc, r_rc, allow_extend in [(0, 0, 0), (1, 0, 1), (0, 1, 0), (1, 1, 1)]:
        args = (q, windows, first, intervals, rolls, 110, 300, 20, 1000, q_rc, 5000, r_rc, allow_extend)
        want = F.filter_tasks(*args)
        code, got = extz2.search_filter_tasks_host(*args)
        assert code == 0 and got.tobytes() == want.tobytes()
        assert ((got["flags"] & F.SKIP) != 0).tolist() == [False, True, True, False, True, False, True]
        assert int(got["q_off"][0]) == (1000 + 110 - 30 if q_rc else 1010) and int(got["q_len"][0]) == 20
        if allow_extend:  # 30 steps from 100; the walk from 280 is clamped at len_r at once
            assert (int(got["r_off"][0]), int(got["r_off"][5])) == ((5000 + 300 - 150, 5000) if r_rc else (5130, 5280))
        else:
            assert int(got["r_off"][0]) == (5000 + 300 - 130 if r_rc else 5110)
    # refusals: nothing is written
    out = np.full(7, 0x55, np.uint8).repeat(32).view(F.TASK)
    for bad, code in [(dict(init_len=0), SDF_ERR_INVALID), (dict(len_q=-1), SDF_ERR_INVALID), (dict(r_off=-5), SDF_ERR_INVALID),
                      (dict(init_len=(1 << 30) + 1), SDF_ERR_UNSUPPORTED), (dict(len_r=1 << 31), SDF_ERR_UNSUPPORTED),
                      (dict(first=np.array([0, 4, 3, 7], np.int64)), SDF_ERR_INVALID), (dict(first=np.array([1, 4, 5, 7], np.int64)), SDF_ERR_INVALID)]:
        kw = dict(q=q, windows=windows, first=first, intervals=intervals, rolls=rolls, len_q=110, len_r=300, init_len=20, q_off=1000, q_rc=0,
                  r_off=5000, r_rc=0, allow_extend=1)
        kw.update(bad)
        assert extz2.search_filter_tasks_host(out=out, **kw)[0] == code, bad
        assert out.tobytes() == b"\x55" * (7 * 32)


def test_host_form_refusals_write_nothing():
    from sedef_amd import extz2
    pool = b"ACGTacgtNNACGTTGCAacgtacgtAC"
    good = np.array([(0, 8, 8, 9, 0, 0), (3, 3, 0, 0, F.Q_RC, 0), (len(pool), 0, 0, len(pool), F.R_RC, 0), (0, 0, 0, 0, F.SKIP, 0)], F.TASK)
    code, got = host(pool, good, F.DEFAULTS)
    assert code == 0 and got.tobytes() == F.filter_pairs(pool, good, **F.DEFAULTS).tobytes() and int(got["flags"][3]) == F.SKIPPED

    def refused(tasks, P=F.DEFAULTS, **kw):
        out = np.full(len(tasks) * 20, 0x55, np.uint8).view(F.REC)
        code, _ = host(pool, tasks, P, out=out, **kw)
        assert out.tobytes() == b"\x55" * (20 * len(tasks))
        return code

    def with_(**kw):
        t = good.copy()
        for k, v in kw.items():
            t[k][1] = v
        return t
    assert refused(with_(q_off=len(pool) + 1)) == SDF_ERR_INVALID
    assert refused(with_(r_off=len(pool) - 2, r_len=3)) == SDF_ERR_INVALID
    assert refused(with_(q_off=-1)) == SDF_ERR_INVALID
    assert refused(with_(q_len=-1)) == SDF_ERR_INVALID
    assert refused(with_(r_off=(1 << 63) - 1, r_len=5)) == SDF_ERR_INVALID
    assert refused(with_(flags=8)) == SDF_ERR_UNSUPPORTED
    assert refused(with_(reserved=1)) == SDF_ERR_UNSUPPORTED
    for name in ("max_error", "max_edit_error", "gap_frequency"):
        for v in (float("nan"), float("inf"), -float("inf")):
            assert refused(good, dict(F.DEFAULTS, **{name: v})) == SDF_ERR_INVALID
    assert refused(good, dict(F.DEFAULTS, reserved=1)) == SDF_ERR_UNSUPPORTED
    lib = extz2.load_library()
    out = np.full(20, 0x55, np.uint8)
    assert lib.sdf_search_filter_host(pool, len(pool), None, good.ctypes.data, 1, out.ctypes.data) == SDF_ERR_INVALID
    assert lib.sdf_search_filter_host(pool, len(pool), extz2.filter_params(), None, 1, out.ctypes.data) == SDF_ERR_INVALID
    assert lib.sdf_search_filter_host(pool, len(pool), extz2.filter_params(), good.ctypes.data, 1, None) == SDF_ERR_INVALID
    assert lib.sdf_search_filter_host(None, 0, None, None, 0, None) == 0  # n == 0
    assert out.tobytes() == b"\x55" * 20
