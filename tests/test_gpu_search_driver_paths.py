"""sdf_search_pair down the paths that its three drawn pairs do not reach: the inputs of driver_model.path_inputs, which
tests/test_search_driver_paths_cpu.py proves to reach them.  Expected values: sdf_search_pair_host's bytes (pinned on the model
there) and, for rounds / windows_run / windows_host, driver_model.rounds -- exact wherever no round of the model needs more
than a starting capacity, a lower bound where one does."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (at collection: before the library brings a HIP runtime of its own along)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import driver_model as DM  # noqa: E402
from test_search_driver_paths_cpu import ALL_IN_ONE, NAMES, hosted, predicted, the_input, within_capacities  # noqa: E402

pytestmark = pytest.mark.gpu

SDF_ERR_OVERFLOW = -5
STATS = ("rounds", "windows_run", "windows_host")


@pytest.fixture(scope="module")
def eng():
    import sedef_amd
    e = sedef_amd.Extz2Engine(0)
    yield e
    e.close()


def ex():
    from sedef_amd import extz2
    return extz2


def drive(eng, name, cap=None, **kw):
    """sdf_search_pair on the input's characters, uploaded as the pool."""
    I = the_input(name)
    eng.pool_upload(I["pool"])
    eng.pool_sync()
    return eng.search_pair(I["q_range"], I["r_range"], cap=cap, **dict(DM.pair_kwargs(ex(), I), **kw))


def same_answer(got, name):
    rc, hits, used, stats = got
    want_hits, want_stats = hosted(name)
    assert rc == 0 and used == len(want_hits)
    assert hits.tobytes() == want_hits.tobytes()
    for f in ("attempted", "jaccard_failed", "interval_failed", "windows_scheduled"):
        assert int(stats[f]) == int(want_stats[f]), f


# (the whole schedule in one round: for the input that exceeds a capacity)
CASES = [(name, rw) for name in NAMES for rw in (1, 64, 0)] + [("b", ALL_IN_ONE), ("e", ALL_IN_ONE)]


@pytest.mark.parametrize("name,round_windows", CASES)
def test_the_driver_is_the_host_form_on_every_path(eng, name, round_windows):
    got = drive(eng, name, round_windows=round_windows)
    same_answer(got, name)
    stats = got[3]
    if name == "c":
        # rounds() is not run here (minutes beyond rounds of one window).  test_c_... of the CPU file: some round starts with
        # more bin entries than the capacity and is repeated; with rounds of one window that is the one round more than the
        # scheduled windows, elsewhere rounds are more than the least that takes every scheduled window once.
        scheduled = int(stats["windows_scheduled"])
        print(name, round_windows, {f: int(stats[f]) for f in stats.dtype.names})
        assert int(stats["windows_host"]) == 0
        if round_windows == 1:
            assert (int(stats["rounds"]), int(stats["windows_run"])) == (scheduled + 1, scheduled + 1)
        else:
            assert int(stats["rounds"]) > -(-scheduled // DM.PAIR_ROUND_WINDOWS) and int(stats["windows_run"]) > scheduled
        return
    R = predicted(name, round_windows)
    print(name, round_windows, {f: int(stats[f]) for f in stats.dtype.names}, {f: R[f] for f in STATS})
    # (the model has the driver's interval and list capacities, and no input here is short of bin entries: exact)
    assert not R["entries_short"]
    assert {f: int(stats[f]) for f in STATS} == {f: R[f] for f in STATS}
    assert within_capacities(R) or name in ("b", "e")  # (the two whose rounds pass the starting interval capacity)
    if name == "e":
        assert int(stats["windows_host"]) >= 1
    if name in ("f", "f_many"):
        assert int(stats["windows_host"]) == 0
    if name == "f_host":
        assert int(stats["windows_host"]) >= 1


def test_pairs_in_succession_on_one_context(eng):
    """The largest input, the smallest, an empty schedule, the largest again: each its own answer, the first and the last
    byte for byte the same; and the smallest on a fresh context as on the used one.  Large and small by the query's length,
    which orders its minimizers: the second run has fewer records in dr_win and dr_first than the first left there.
    (c, whose runs take seconds each, is left to its own cases.)"""
    by_size = sorted((n for n in NAMES if n[0] not in "jc"), key=lambda n: the_input(n)["q_range"][1])
    small, large = by_size[0], by_size[-1]
    assert small == "e" and large[0] == "f" and the_input(large)["q_range"][1] > 15 * the_input(small)["q_range"][1]
    runs = [drive(eng, n) for n in (large, small, "j_lower", large)]
    for got, n in zip(runs, (large, small, "j_lower", large)):
        same_answer(got, n)
    assert runs[0][1].tobytes() == runs[3][1].tobytes() and runs[0][3].tobytes() == runs[3][3].tobytes()
    assert not any(int(runs[2][3][f]) for f in runs[2][3].dtype.names)
    import sedef_amd
    fresh = sedef_amd.Extz2Engine(0)
    try:
        alone = drive(fresh, small)
    finally:
        fresh.close()
    assert alone[1].tobytes() == runs[1][1].tobytes() and alone[3].tobytes() == runs[1][3].tobytes()


def test_nothing_behind_out_cap_for_a_pair_whose_rounds_grew(eng):
    """The raw call with cap exact and one short, canary records behind the buffer; the pair's first round was short of
    intervals, and its second made the device list grow with a record in it."""
    kinds = [ev[0] for ev in predicted("b", 0)["events"]]
    assert "partial" in kinds and kinds.count("found_grew") >= 2
    extz2, I = ex(), the_input("b")
    want = hosted("b")[0]
    eng.pool_upload(I["pool"])
    eng.pool_sync()
    kw = DM.pair_kwargs(extz2, I)
    limit = np.ascontiguousarray(I["limit"], np.int32)
    P = extz2._PairParams(I["k"], I["w"], 1, 1, I["init_len"], 0, kw["filter"], kw["extend"], limit.ctypes.data, len(limit), 0, 0)
    ranges = [extz2._MinimRange(*I["q_range"]), extz2._MinimRange(*I["r_range"])]
    for cap in (len(want), len(want) - 1):
        out = np.full((cap + 4) * 6, -1, np.int32)
        need, stats = C.c_size_t(0), np.zeros(1, extz2.PAIR_STATS_DTYPE)
        rc = eng.lib.sdf_search_pair(eng.ctx, C.byref(ranges[0]), C.byref(ranges[1]), C.byref(P), out.ctypes.data, cap, C.byref(need),
                                     stats.ctypes.data)
        assert need.value == len(want) and (out[cap * 6:] == -1).all()
        if cap == len(want):
            assert rc == 0 and out[:cap * 6].tobytes() == want.tobytes() and int(stats["rounds"][0]) == predicted("b", 0)["rounds"]
        else:
            assert rc == SDF_ERR_OVERFLOW and (out == -1).all()
