"""CPU: search seeding -- the reference intervals of every query window (include/sedef_hip.h: sdf_search_windows) -- pinned on
the reference (tests/golden/search_windows_kat.json.gz, written by tests/golden/make_golden_search_windows.py from the front
half of the reference's own search() with its Index and SlidingMap):
  * tests/search_model.py, the seven steps in plain Python, gives the fixture's query sizes, candidates and intervals;
  * sdf_search_windows_host, the same steps in C++ behind the C ABI (no context, no GPU), gives the model's records, one for
    one, and keeps the overflow protocol and the refusals of the header."""
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
import search_model as S  # noqa: E402

SDF_ERR_UNSUPPORTED, SDF_ERR_INVALID, SDF_ERR_OVERFLOW = -3, -4, -5


def load_fixture():
    with gzip.open(os.path.join(ROOT, "tests", "golden", "search_windows_kat.json.gz"), "rb") as f:
        return json.loads(f.read().decode())


@pytest.fixture(scope="module")
def fixture():
    return load_fixture()


def case_sequences(c):
    """(query, reference as the reference program sees it) of a fixture case."""
    q = c["q"].encode()
    if c["same"]:
        return q, q
    r = c["r"].encode()
    return q, M.rev_comp(r) if c["r_rc"] else r


def case_arrays(c):
    """A case's query minimizers in loc order and its reference records in index order, by tests/minim_model.py."""
    qs, rs = case_sequences(c)
    q = S.records(M.get_minimizers(qs, c["k"], c["w"], bool(c["sl"])))
    r = q if c["same"] else S.records(M.get_minimizers(rs, c["k"], c["w"], bool(c["sl"])))
    return q, S.index_order(r)


def case_args(c):
    return dict(r_threshold=c["threshold"], len_q=len(c["q"]), init_len=c["init_len"], same_genome=c["same_genome"],
                uppercase_seeds=c["uppercase_seeds"], limit=c["limit"])


def case_expected(c):
    """(first, windows without n_members / n_gathered, intervals) as the fixture has them."""
    first, out = [0], []
    for qsz, flags, cand, T in c["windows"]:
        out += T
        first.append(len(out))
    return np.array(first, np.int64), np.array(out, np.int64).reshape(-1, 2)


@pytest.fixture(scope="module")
def modelled(fixture):
    """The model's answer for every case of the fixture, computed once."""
    return [S.search_windows(*case_arrays(c), **case_args(c), detail=True) for c in fixture["cases"]]


def host(q, r_sorted, **kw):
    from sedef_amd import extz2
    return extz2.search_windows_host(q, r_sorted, **kw)


def same_records(got, want):
    gf, gw, go = got
    wf, ww, wo = want
    assert np.array_equal(np.asarray(gf, np.int64), wf), (gf[:10], wf[:10])
    assert gw.tobytes() == ww.tobytes(), [(i, gw[i], ww[i]) for i in np.flatnonzero(gw != ww)[:5]]
    assert go.tobytes() == wo.tobytes(), [(i, go[i], wo[i]) for i in np.flatnonzero(go != wo)[:5]]


def test_fixture_holds_the_cases_it_promises(fixture):
    cases = fixture["cases"]
    windows = [w for c in cases for w in c["windows"]]
    assert 3 * sum(len(w[3]) > 0 for w in windows) >= len(windows)
    assert sum(len(w[3]) >= 2 for w in windows) >= 50
    assert {w[1] for w in windows} == {0, S.SHORT, S.NOLIMIT}
    assert any(c["r_rc"] for c in cases) and any(c["same_genome"] for c in cases)
    assert {0, 1} == {c["uppercase_seeds"] for c in cases} and any(c["threshold"] < 100 for c in cases)
    both = 0
    for c in cases:
        both += {1, 2} <= {m[2] for m in M.get_minimizers(c["q"].encode(), c["k"], c["w"], bool(c["sl"]))}
    assert both >= 20


def test_model_gives_the_fixture(fixture, modelled):
    dup = 0
    for c, (first, windows, out, cands) in zip(fixture["cases"], modelled):
        want_first, want_out = case_expected(c)
        assert len(windows) == c["nq"], c["name"]
        assert windows["query_size"].tolist() == [w[0] for w in c["windows"]], c["name"]
        assert (windows["flags"] & ~np.uint32(S.WIDE)).tolist() == [w[1] for w in c["windows"]], c["name"]
        assert cands == [w[2] for w in c["windows"]], c["name"]
        assert np.array_equal(first, want_first), c["name"]
        assert np.array_equal(np.stack([out["start"], out["end"]], 1), want_out), c["name"]
        dup += int(np.sum((windows["query_size"] < windows["n_members"]) & (windows["flags"] == 0)))
    assert dup >= 20  # (windows with one key at several members)


def test_host_form_gives_the_model_record_for_record(fixture, modelled):
    for c, (first, windows, out, cands) in zip(fixture["cases"], modelled):
        code, gf, gw, go, used = host(*case_arrays(c), **case_args(c))
        assert code == 0 and used == len(out) == int(gf[-1]), c["name"]
        same_records((gf, gw, go), (first, windows, out))


def wide_arrays(n_gathered, n_members=40):
    """A query of n_members minimizers 5 bases apart with distinct hashes, the first of which has a group of n_gathered - (n_members
    - 1) reference records and the others one each: n_gathered in all from window 0."""
    q = S.records([(100 + j, 5 * j, 0) for j in range(n_members)])
    big = n_gathered - (n_members - 1)
    rows = [(100, 3 * t, 0) for t in range(big)] + [(100 + j, 7 * j + 1, 0) for j in range(1, n_members)]
    return q, S.index_order(S.records(rows))


def test_host_form_completes_wide_windows():
    for n_gathered in (4095, 4096, 4097, 6000):
        q, r = wide_arrays(n_gathered)
        kw = dict(r_threshold=1 << 31, len_q=100000, init_len=1000, same_genome=0, uppercase_seeds=1, limit=[1] + [3] * 60)
        want = S.search_windows(q, r, **kw)
        assert bool(want[1]["flags"][0] & S.WIDE) == (n_gathered > S.MAX_GATHER) and int(want[1]["n_gathered"][0]) == n_gathered
        assert want[1]["n_candidates"][0] > 3000 and want[0][1] > 0
        code, gf, gw, go, used = host(q, r, **kw)
        assert code == 0
        same_records((gf, gw, go[:used]), want)
    # 1,025 members: WIDE by the other count
    q = S.records([(7 + (j % 3), j, 0) for j in range(1200)])
    r = S.index_order(S.records([(7, 50, 0), (8, 60, 0), (7, 90, 0)]))
    kw = dict(r_threshold=1 << 31, len_q=5000, init_len=1024, same_genome=0, uppercase_seeds=0, limit=[1, 1, 1, 2])
    want = S.search_windows(q, r, **kw)
    assert want[1]["n_members"][0] == 1025 and want[1]["flags"][0] == S.WIDE and want[1]["query_size"][0] == 3
    assert want[1]["n_members"][1] == 1025 and want[1]["n_members"][176] == 1024 and want[1]["flags"][176] == 0
    code, gf, gw, go, used = host(q, r, **kw)
    assert code == 0
    same_records((gf, gw, go[:used]), want)


def test_host_form_overflow_protocol(fixture, modelled):
    from sedef_amd import extz2
    c = fixture["cases"][0]
    first, windows, out, _ = modelled[0]
    need = len(out)
    assert need > 10
    q, r = case_arrays(c)
    for cap in (need - 1, need, 0):
        buf = np.frombuffer(b"\xEE" * (8 * (need + 8)), extz2.SEARCH_INTERVAL_DTYPE).copy()
        code, gf, gw, go, used = host(q, r, cap=cap, out=buf, **case_args(c))
        assert used == need and np.array_equal(gf.astype(np.int64), first) and gw.tobytes() == windows.tobytes()
        if cap >= need:
            assert code == 0 and buf[:need].tobytes() == out.tobytes()
            assert buf[need:].tobytes() == b"\xEE" * (8 * 8)
        else:
            assert code == SDF_ERR_OVERFLOW
            assert buf.tobytes() == b"\xEE" * (8 * (need + 8))  # nothing is written to out


def test_host_form_refusals():
    import ctypes as C

    from sedef_amd import extz2
    lib = extz2.load_library()
    q, r = wide_arrays(100)
    kw = dict(r_threshold=1 << 31, len_q=100000, init_len=1000, same_genome=0, uppercase_seeds=1, limit=[1] + [3] * 60)
    assert host(q, r, **kw)[0] == 0
    assert host(q, r, **dict(kw, init_len=0))[0] == SDF_ERR_INVALID
    assert host(q, r, **dict(kw, init_len=-5))[0] == SDF_ERR_INVALID
    assert host(q, r, **dict(kw, init_len=(1 << 30) + 1))[0] == SDF_ERR_UNSUPPORTED
    assert host(q, r, **dict(kw, limit=[0, 3, 0, 3]))[0] == SDF_ERR_UNSUPPORTED  # (limit[2] < 1; limit[0] is never read)
    assert host(q, r, **dict(kw, limit=[0, 3, -1]))[0] == SDF_ERR_UNSUPPORTED
    code, first, windows, out, used = host(q, r, **dict(kw, limit=[]))  # no table: every window NOLIMIT
    assert code == 0 and used == 0 and set(windows["flags"].tolist()) == {S.NOLIMIT}
    code, first, windows, out, used = host(q[:0], r, **kw)  # nq == 0
    assert code == 0 and used == 0 and first.tolist() == [0]
    # null pointers, straight at the symbol
    first, windows, used = np.zeros(len(q) + 1, np.uint64), np.zeros(len(q), extz2.SEARCH_WINDOW_DTYPE), C.c_size_t(0)
    limit = np.array(kw["limit"], np.int32)
    good = [q.ctypes.data, len(q), 100000, r.ctypes.data, len(r), 1 << 31, 1000, 0, 1, limit.ctypes.data, len(limit), first.ctypes.data,
            windows.ctypes.data, None, 0, C.byref(used)]
    assert lib.sdf_search_windows_host(*good) == SDF_ERR_OVERFLOW and used.value > 0
    for at in (0, 3, 9, 11, 12, 15):
        bad = list(good)
        bad[at] = None
        assert lib.sdf_search_windows_host(*bad) == SDF_ERR_INVALID, at
    bad = list(good)
    bad[14] = 5  # cap > 0 without out
    assert lib.sdf_search_windows_host(*bad) == SDF_ERR_INVALID


def test_library_exports_the_entry_points_and_record_sizes():
    from sedef_amd import extz2
    lib = extz2.load_library()
    for name in ("sdf_search_windows", "sdf_search_windows_device", "sdf_search_windows_host"):
        assert hasattr(lib, name), name
    assert extz2.SEARCH_WINDOW_DTYPE == S.WINDOW and extz2.SEARCH_INTERVAL_DTYPE == S.INTERVAL and extz2.MINIMIZER_DTYPE == S.MINIMIZER
    header = open(os.path.join(ROOT, "include", "sedef_hip.h")).read()
    assert "#define SDF_SEARCH_MAX_MEMBERS %d" % extz2.SEARCH_MAX_MEMBERS in header
    assert "#define SDF_SEARCH_MAX_GATHER %d" % extz2.SEARCH_MAX_GATHER in header
    assert (extz2.SEARCH_SHORT, extz2.SEARCH_NOLIMIT, extz2.SEARCH_WIDE) == (S.SHORT, S.NOLIMIT, S.WIDE)
    for name in ("search_windows_raw", "search_windows_device", "search_windows"):
        assert callable(getattr(extz2.Extz2Engine, name))
