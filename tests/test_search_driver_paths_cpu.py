"""The inputs that take sdf_search_pair down the paths its three drawn pairs do not reach (driver_model.path_inputs), each
proven here, on the CPU, to reach its path: from driver_model.rounds -- the driver's loop in Python, with the driver's interval
and list capacities -- and the host forms alone.  tests/test_gpu_search_driver_paths.py drives the device with them.

For every input sdf_search_pair_host equals driver_model.initial_search byte for byte, and rounds() equals both.

What is not here, and why:
  the interval capacity's REPEAT branch (back.intervals > cap_iv with frontier == 0): intervals alone cannot take it.  The
      round's first scheduled window is the first of the slice, so its records are first[i0 + 1] in number, and a window has
      no more intervals than candidates, no more candidates than it gathered, and is WIDE -- without an interval -- beyond
      SDF_SEARCH_MAX_GATHER = 4,096 = SDF_PAIR_INTERVALS_START gathered: the first window's records always fit.  The branch is
      taken only by a round whose first window is left to the host (FOUND_WIDE, say) while the rest of its slice needs more
      intervals than the capacity AS RAISED SO FAR; no input here has such a round (test_no_input_repeats_a_round says so from
      the model, so that a change of the inputs that reaches it is noticed), and the branch stays unrun;
  the three stats of c (the entries capacity) at rounds of more than one window: rounds() -- Python's accept over every
      interval of every round -- takes minutes there; c's answer is compared at every round size, its stats exactly at
      rounds of one window and against the least a driver can take elsewhere."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import driver_model as DM  # noqa: E402
import found_model as FM  # noqa: E402

ALL_IN_ONE = 1 << 20  # a round_windows that puts the whole schedule into one round
NAMES = tuple(DM.path_inputs())
# (name, round_windows) for which rounds() runs: not c beyond rounds of one window (the module's docstring), and f_host's
# whole schedule in one round, a minute of long growths in every window of the segment, is left out as well
MODELLED = [(name, rw) for name in NAMES for rw in (1, 64, ALL_IN_ONE)
            if (name != "c" or rw == 1) and (name != "f_host" or rw != ALL_IN_ONE)]
# one window with 17 long growths needs 17 reference copies of a segment of more than SDF_EXTEND_MAX_GROW records, 8.9 kb at
# k = 8, w = 4: f_host alone is larger than the few tens of kilobases the others keep to
MAX_POOL = {"f_host": 180000}
_inputs, _modelled, _hosted, _rounds = {}, {}, {}, {}


def ex():
    from sedef_amd import extz2
    return extz2


def the_input(name):
    if not _inputs:
        _inputs.update(DM.path_inputs())
    return _inputs[name]


def modelled(name):
    if name not in _modelled:
        _modelled[name] = DM.initial_search(ex(), the_input(name))
    return _modelled[name]


def hosted(name):
    """sdf_search_pair_host's answer: (hits, stats)."""
    if name not in _hosted:
        I = the_input(name)
        rc, hits, used, stats = ex().search_pair_host(I["pool"], I["q_range"], I["r_range"], **DM.pair_kwargs(ex(), I))
        assert rc == 0 and used == len(hits)
        _hosted[name] = (hits, stats)
    return _hosted[name]


def predicted(name, round_windows):
    """rounds() with the driver's capacities: its three stats are the driver's, exactly, unless entries_short."""
    key = (name, round_windows or DM.PAIR_ROUND_WINDOWS)
    if key not in _rounds:
        _rounds[key] = DM.rounds(ex(), the_input(name), round_windows, capacities=True)
    return _rounds[key]


def within_capacities(R):
    """No round of the model needs more than the driver's starting capacities."""
    return all(p[2] <= DM.PAIR_INTERVALS_START and p[3] <= DM.PAIR_ENTRIES_START for p in R["per_round"])


def test_the_constants_are_the_librarys():
    extz2 = ex()
    header = open(os.path.join(ROOT, "include", "sedef_hip.h")).read()
    for name in ("ROUND_WINDOWS", "INTERVALS_START", "ENTRIES_START", "LONG_MAX", "LONG_BATCH"):
        assert "#define SDF_PAIR_%s %d\n" % (name, getattr(extz2, "PAIR_" + name)) in header, name
    assert extz2.PAIR_INTERVALS_START >= extz2.SEARCH_MAX_GATHER  # (a window's records always fit: the module's docstring)
    import ctypes as C
    assert C.sizeof(extz2._PairParams) == 120 and extz2.PAIR_STATS_DTYPE.itemsize == 56


@pytest.mark.parametrize("name", NAMES)
def test_pair_host_is_the_model(name):
    want = modelled(name)
    hits, stats = hosted(name)
    assert hits.tobytes() == want["hits"].tobytes()
    for f in ("attempted", "jaccard_failed", "interval_failed"):
        assert int(stats[f]) == want["count"][f], f
    assert int(stats["windows_scheduled"]) == len(want["ran"]) and int(stats["rounds"]) == 0
    assert len(the_input(name)["pool"]) <= MAX_POOL.get(name, 40000)


@pytest.mark.parametrize("name,round_windows", MODELLED)
def test_the_rounds_are_the_model(name, round_windows):
    """rounds() reports what initial_search reports, whatever the round."""
    want, R = modelled(name), predicted(name, round_windows)
    assert R["hits"].tobytes() == want["hits"].tobytes() and R["count"] == want["count"]
    assert R["sched"] == want["ran"] and R["windows_run"] >= R["scheduled"] and not R["entries_short"]
    if round_windows == 1 and R["windows_host"] == 0:
        repeats = [ev[0] for ev in R["events"]].count("entries")
        assert R["rounds"] == R["windows_run"] == R["scheduled"] + repeats


def test_b_a_round_short_of_intervals_is_taken_as_far_as_its_records_go():
    """Rounds of 64 windows and the whole schedule in one: a round needs more intervals than the starting capacity, its first
    windows' records lie below it, and nothing else stops it there -- the driver accepts those windows and doubles the capacity
    beyond the need (the model's "partial" event)."""
    for round_windows in (64, ALL_IN_ONE):
        R = predicted("b", round_windows)
        short = [p for p in R["per_round"] if p[2] > DM.PAIR_INTERVALS_START]
        assert short and all(p[6] == 0 for p in R["per_round"]) and R["windows_host"] == 0
        assert [ev[0] for ev in R["events"]].count("partial") >= 1
        assert all(p[3] <= DM.PAIR_ENTRIES_START for p in R["per_round"])
    # from first[]: in the first round the first scheduled windows' records end below the capacity, a later one's beyond it
    extz2, I = ex(), the_input("b")
    P = DM.Pair(extz2, I)
    sched = R["sched"]
    rc, first, windows, T, used = extz2.search_windows_found_host(P.q, P.r_sorted, P.threshold, P.len_q, P.init_len, 0, 1, P.limit,
                                                                  FM.found_records([]), np.zeros(len(P.q), np.uint32))
    assert rc == 0 and not (windows["flags"] & (DM.WIN_WIDE | DM.WIN_FOUND_WIDE)).any()
    ends = [int(first[i + 1]) - int(first[sched[0]]) for i in sched[:64]]
    assert ends[0] <= DM.PAIR_INTERVALS_START < ends[-1]


def test_d_the_device_list_grows_with_records_in_it():
    """pair_sync_found with nf > 0 and a capacity that is short: the whole mirror is uploaded again.  From the constants and
    the rule 2 * want + 1024: the first round sizes the list for the starting interval capacity; a round that was short of
    intervals doubles that capacity beyond its need, and the next round's nf + capacity passes the list's."""
    first_cap = 2 * DM.PAIR_INTERVALS_START + 1024
    for name, round_windows in (("b", 64), ("b", ALL_IN_ONE), ("e", 1), ("e", 64)):
        R = predicted(name, round_windows)
        grew = [ev for ev in R["events"] if ev[0] == "found_grew"]
        assert grew[0] == ("found_grew", 0, DM.PAIR_INTERVALS_START, 0)
        assert len(grew) >= 2 and grew[1][1] > 0 and grew[1][2] > grew[1][3] == first_cap, (name, grew)
        # ... and the want is nf + twice the intervals of the round that was short
        partial = [ev for ev in R["events"] if ev[0] == "partial"][0]
        assert grew[1][2] == grew[1][1] + 2 * partial[2]
    assert predicted("e", 1)["events"][2][1] > 500  # (hundreds of records uploaded again)


def test_no_input_repeats_a_round():
    """(the module's docstring: the repeat branch stays unrun)"""
    for name, round_windows in MODELLED:
        if round_windows != ALL_IN_ONE:
            assert not [ev for ev in predicted(name, round_windows)["events"] if ev[0] == "repeat"], name


def test_f_long_growths_are_finished_inside_a_round():
    """A hit grew by more than SDF_EXTEND_MAX_GROW records; f: never more than SDF_PAIR_LONG_MAX candidates a round; f_many:
    rounds with more, whose first window's are still among those finished (the module's docstring) -- no window for the host."""
    extz2 = ex()
    for name in ("f", "f_many"):
        assert modelled(name)["seen"]["max_grow"] > extz2.EXTEND_MAX_GROW and len(modelled(name)["hits"]) >= 1
        for round_windows in (1, 64):
            R = predicted(name, round_windows)
            longs = [p[7] for p in R["per_round"]]
            assert max(longs) >= 1 and R["windows_host"] == 0
            # a round with a long growth accepted its window: the growth was finished there
            assert any(p[7] >= 1 and p[5] >= 1 and p[4] < len(modelled(name)["found"]) for p in R["per_round"])
            if round_windows == 64:
                assert (max(longs) <= DM.PAIR_LONG_MAX) == (name == "f"), (name, max(longs))


def test_f_host_a_window_with_more_long_growths_than_a_round_finishes():
    """The window at the segment's start has 17 long growths or more: the device finishes SDF_PAIR_LONG_MAX, the window is
    incomplete and the host takes it, whatever the round."""
    extz2 = ex()
    assert modelled("f_host")["seen"]["max_grow"] > extz2.EXTEND_MAX_GROW
    for round_windows in (1, 64):
        R = predicted("f_host", round_windows)
        assert R["windows_host"] >= 1 and not R["events"][1:]
        handed = [p for p in R["per_round"] if p[6] & DM.INCOMPLETE]
        assert handed and all(p[7] > DM.PAIR_LONG_MAX for p in handed)  # (handed over for its long growths, nothing else)
    assert modelled("f_host")["seen"]["max_meeting"] <= FM.MAX_FOUND


def test_c_the_found_list_needs_more_bin_entries_than_the_index_starts_with():
    """From initial_search's found list alone: the records found before the 65th scheduled window from the end have more
    bin entries than SDF_PAIR_ENTRIES_START, so with rounds of at most 64 windows some round starts with such a list -- and is
    repeated.  With rounds of one window the model says the rest: one repeat, no window for the host, no round short of
    intervals; and the device list grows with thousands of records in it."""
    extz2, want = ex(), modelled("c")
    before = want["nf_before"][-65]
    assert extz2.found_entries(FM.found_records(want["found"][:before])) > DM.PAIR_ENTRIES_START
    assert extz2.found_entries(FM.found_records(want["found"])) <= 2 * DM.PAIR_ENTRIES_START  # (one doubling is enough)
    assert want["seen"]["max_meeting"] <= FM.MAX_FOUND
    R = predicted("c", 1)
    kinds = [ev[0] for ev in R["events"]]
    assert kinds.count("entries") == 1 and "partial" not in kinds and "repeat" not in kinds and not R["entries_short"]
    assert (R["rounds"], R["windows_run"], R["windows_host"]) == (R["scheduled"] + 1, R["scheduled"] + 1, 0)
    grew = [ev for ev in R["events"] if ev[0] == "found_grew"]
    assert len(grew) == 2 and grew[1][1] > 4000 and grew[1][3] == 2 * DM.PAIR_INTERVALS_START + 1024


def test_i_parse_hits_drops_a_drawn_hit():
    want = modelled("i")
    assert want["seen"]["dropped"] >= 1 and len(want["found"]) == len(want["hits"]) + want["seen"]["dropped"]


def test_the_near_records_of_a_window_answer_as_the_whole_list():
    """Pair.window asks only the records that can cover a member of the window; the whole list answers the same."""
    from test_search_driver_cpu import INPUTS
    extz2 = ex()
    for which in INPUTS[:2]:
        P = DM.Pair(extz2, DM.inputs(*which))
        found = []
        for i in DM.greedy_schedule(P.q, P.min_read_size, 1):
            loc = int(P.q["loc"][i])
            whole = P.walk.window(i, FM.RecordList(found, len(found)).excluded)
            near = [R for R in found if R[0] <= loc + P.init_len and R[1] > loc]
            assert whole == P.walk.window(i, FM.RecordList(near, len(near)).excluded)
            for R in found[::7]:  # is_overlap, at ranges that earlier hits name
                args = (loc, loc + P.init_len, R[2], R[2] + P.init_len, P.min_read_size)
                assert FM.RecordList(found, len(found)).is_overlap(*args) == FM.RecordList(near, len(near)).is_overlap(*args)
            P.window(i, found, dict(attempted=0, jaccard_failed=0, interval_failed=0))
        assert len(found) > 50


def test_e_a_window_meets_more_records_than_the_device_takes():
    """FOUND_WIDE with debug_host_every = 0: the host takes the window, and the round behind it starts with its records."""
    want = modelled("e")
    assert want["seen"]["max_meeting"] > FM.MAX_FOUND
    extz2 = ex()
    assert extz2.SEARCH_MAX_FOUND == FM.MAX_FOUND
    for round_windows in (1, 64):
        R = predicted("e", round_windows)
        assert R["windows_host"] >= 1
        handed = [k for k, p in enumerate(R["per_round"]) if p[6] & DM.INCOMPLETE]
        assert handed
        k = handed[0]
        window = R["sched"][R["per_round"][k][0] + R["per_round"][k][5]]
        mine = [tuple(int(x) for x in h)[1:5] for h in want["hits"] if h["window"] == window]
        assert mine and k + 1 < len(R["found_at"]) and all(h in R["found_at"][k + 1] for h in mine)
        assert not any(h in R["found_at"][k] for h in mine)


def test_g_the_query_at_an_offset_and_on_the_other_strand():
    for name in ("g_off", "g_off_rrc", "g_qrc", "g_qrc_rrc"):
        I = the_input(name)
        assert len(modelled(name)["hits"]) >= 5, name
        assert (I["q_range"][0] != 0) == name.startswith("g_off") and bool(I["q_range"][2]) == name.startswith("g_qrc")
        assert bool(I["r_range"][2]) == name.endswith("rrc")
    # the flag matters: the same characters searched on the strand the pool holds give another answer
    I = the_input("g_qrc")
    other = dict(I, q_range=I["q_range"][:2] + (0,))
    rc, hits, _, _ = ex().search_pair_host(other["pool"], other["q_range"], other["r_range"], **DM.pair_kwargs(ex(), other))
    assert rc == 0 and hits.tobytes() != hosted("g_qrc")[0].tobytes()


def test_h_case_and_parameters_move_the_schedule():
    base = modelled("h")
    assert (base["q"]["status"] == 1).any() and (base["q"]["status"] == 2).any()
    skipped = [i for i in DM.greedy_schedule(base["q"], 60, False) if base["q"]["status"][i] != 0]
    assert skipped  # (some window the default skips by its status)
    assert len(base["hits"]) >= 5
    for name in ("h_all_seeds", "h_one_case", "h_max_error"):
        other = modelled(name)
        assert len(other["hits"]) >= 5
        assert [int(other["q"]["loc"][i]) for i in other["ran"]] != [int(base["q"]["loc"][i]) for i in base["ran"]], name
    assert not (modelled("h_one_case")["q"]["status"] == 1).any()


def test_j_empty_schedules():
    for name in ("j_short", "j_lower"):
        want = modelled(name)
        hits, stats = hosted(name)
        assert want["ran"] == [] and len(hits) == 0 and not any(int(stats[f]) for f in stats.dtype.names), name
        R = predicted(name, 64)
        assert (R["rounds"], R["windows_run"], R["windows_host"], R["scheduled"]) == (0, 0, 0, 0)
    I = the_input("j_short")
    assert I["q_range"][1] == I["k"] - 1
    assert len(modelled("j_lower")["q"]) > 100 and (modelled("j_lower")["q"]["status"] != 0).all()


@pytest.mark.parametrize("round_windows", (1, 2, 7, 64))
def test_the_old_inputs_rounds_are_the_model(round_windows):
    from test_search_driver_cpu import INPUTS, modelled as old
    for which in INPUTS:
        I, want = old(which)
        R = DM.rounds(ex(), I, round_windows)
        assert R["hits"].tobytes() == want["hits"].tobytes() and R["count"] == want["count"]
        assert within_capacities(R) and R["windows_host"] == 0
