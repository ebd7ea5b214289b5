"""The search driver's host forms: sdf_search_pair_host (initial_search window by window) and sdf_search_accept_host (the
acceptance step of a round).

The reference's search.cc needs Boost and cannot be built here, so parity is against tests/driver_model.py: the
reference's loop in Python, composed of parts that are each pinned on the reference by their own tests (minim_model, found_model,
and the host forms of roll, filter and extend against their goldens).  Every comparison is exact."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import driver_model as DM  # noqa: E402
import found_model as FM  # noqa: E402

SDF_ERR_UNSUPPORTED, SDF_ERR_INVALID, SDF_ERR_OVERFLOW = -3, -4, -5
# (seed, same_genome, init_len, reverse-complemented reference); the seeds chosen here, on the CPU, so that the asserts of
# test_the_inputs_show_what_they_must hold
INPUTS = ((11, 0, 60, False), (13, 1, 90, False), (29, 0, 75, True))
_runs = {}


def ex():
    from sedef_amd import extz2
    return extz2


def modelled(which):
    if which not in _runs:
        I = DM.inputs(*which)
        _runs[which] = (I, DM.initial_search(ex(), I))
    return _runs[which]


def host_pair(I, cap=None, **change):
    extz2 = ex()
    kw = dict(k=I["k"], w=I["w"], min_read_size=I["init_len"], same_genome=I["same_genome"], limit=I["limit"],
              extend=extz2.extend_params(same_genome=bool(I["same_genome"]), max_sd_size=int(2.5 * I["init_len"])), cap=cap)
    kw.update(change)
    return extz2.search_pair_host(I["pool"], I["q_range"], I["r_range"], **kw)


# ---- 1. sdf_search_pair_host against the model ----

@pytest.mark.parametrize("which", INPUTS)
def test_pair_host_is_the_model(which):
    I, want = modelled(which)
    rc, hits, used, stats = host_pair(I)
    assert rc == 0 and used == len(want["hits"])
    assert hits.tobytes() == want["hits"].tobytes()
    for f in ("attempted", "jaccard_failed", "interval_failed"):
        assert int(stats[f]) == want["count"][f], f
    assert int(stats["windows_scheduled"]) == len(want["ran"]) and int(stats["rounds"]) == 0
    # out one short: the overflow code, the need, nothing written
    if used:
        rc, none, need, _ = host_pair(I, cap=used - 1)
        assert rc == SDF_ERR_OVERFLOW and need == used and len(none) == 0


def test_the_inputs_show_what_they_must():
    seen = dict(failed_in_window=0, failed_by_earlier=0, lost=0, dropped=0)
    for which in INPUTS:
        I, want = modelled(which)
        assert len(want["hits"]) >= 5, which
        for f in seen:
            seen[f] += want["seen"][f]
    assert seen["failed_in_window"] >= 1 and seen["failed_by_earlier"] >= 1 and seen["lost"] >= 1, seen
    # (a hit dropped by parse_hits: whether a drawn input shows one is printed, not asserted -- the hand-made rounds below carry
    # identical and contained hits, and assert that they are dropped)
    print("hits dropped by parse_hits on the drawn inputs:", seen["dropped"])


@pytest.mark.parametrize("which", INPUTS)
def test_fact_1_the_schedule_does_not_depend_on_the_hits(which):
    I, want = modelled(which)
    assert want["ran"] == DM.greedy_schedule(want["q"], want["min_read_size"], True)
    lengths = want["hits"]["query_end"] - want["hits"]["query_start"]
    assert (lengths >= want["min_read_size"]).all()


# ---- 2. sdf_search_accept_host against the model, on hand-made rounds ----

HIT = (900, 1300, 4900, 5300)  # a hit of the window at 1000: 400 bases on either axis
iv = DM.Round.iv


def hand_made_rounds():
    """(name, Round, found rows, out rows, found_cap, out_cap, window_base, what the model's answer must show)."""
    out = []
    some_found, some_out = [(1, 50, 1, 50), (10, 20, 10, 20)], [(3, 1, 50, 1, 50, 9)]

    def add(name, R, shows, found=some_found, outs=some_out, found_cap=None, out_cap=None, base=0):
        out.append((name, R, list(found), list(outs), found_cap, out_cap, base, shows))

    add("an empty round", DM.Round(), lambda s, f, o: s["frontier"] == 0 and s["nf"] == 2 and s["n_out"] == 1 and s["flags"] == 0)
    add("a window with no interval", DM.Round().window(1000).window(2000, [iv(HIT)]),
        lambda s, f, o: s["frontier"] == 2 and s["nf"] == 3 and o[-1] == (1,) + HIT + (7,))
    add("every way an interval is not a hit",
        DM.Round().window(1000, [iv(HIT, jaccard=-1), iv(HIT, verdict=1), iv(HIT, f1=1), iv(HIT, f1=2), iv(HIT, f1=8), iv(HIT, f2=2),
                                 iv(HIT, hflags=1), iv(HIT, hflags=4), iv(HIT, hflags=6), iv(HIT, ref=(9000, 9100), hflags=2), iv(HIT, f1=4, f2=4,
                                                                                                                               ref=(9500, 9600))]),
        lambda s, f, o: (s["attempted"], s["jaccard_failed"], s["interval_failed"]) == (11, 1, 1) and s["nf"] == 4)
    # is_overlap inside a window: the first interval's hit is kept, the second is tested against it
    add("rule 2 decides", DM.Round().window(1000, [iv((1000, 1100, 5000, 5100)), iv(HIT, ref=(5000, 5100))]),
        lambda s, f, o: s["interval_failed"] == 1 and s["nf"] == 3)
    add("rule 3 decides", DM.Round().window(1000, [iv((990, 1120, 4990, 5120)), iv(HIT, ref=(5030, 5130))]),
        lambda s, f, o: s["interval_failed"] == 0 and s["nf"] == 4)
    add("rule 4 decides: 1", DM.Round().window(1000, [iv(HIT), iv(HIT, ref=(5150, 5400))]), lambda s, f, o: s["interval_failed"] == 1 and s["nf"] == 3)
    add("rule 4 decides: 0", DM.Round().window(1000, [iv(HIT), iv((800, 1400, 5200, 5800), ref=(5250, 5400))]),
        lambda s, f, o: s["interval_failed"] == 0 and s["nf"] == 4)
    add("an interval that cannot be kept is still failed by the window's own hit",
        DM.Round().window(1000, [iv(HIT), iv(HIT, ref=(5000, 5100), f1=2)]), lambda s, f, o: s["interval_failed"] == 1 and s["nf"] == 3)
    # parse_hits: identical hits drop each other and stay in found; containment with equal edges
    add("identical hits", DM.Round().window(1000, [iv(HIT), iv(HIT, ref=(9000, 9100))]), lambda s, f, o: s["nf"] == 4 and s["n_out"] == 1)
    add("containment with equal edges", DM.Round().window(1000, [iv((900, 1200, 4900, 5300), ref=(9000, 9100)), iv(HIT, ref=(9400, 9500)),
                                                                 iv(HIT[:3] + (5301,), ref=(9200, 9300))]),
        lambda s, f, o: s["nf"] == 5 and s["n_out"] == 2 and o[-1][1:5] == HIT[:3] + (5301,), base=40)
    # the frontier
    add("q_end == qs_j does not reach", DM.Round().window(1000, [iv((900, 2000, 4900, 6000))]).window(2000, [iv((1900, 2400, 7000, 7500))]),
        lambda s, f, o: s["frontier"] == 2 and s["nf"] == 4)
    add("q_end == qs_j + 1 reaches", DM.Round().window(1000, [iv((900, 2001, 4900, 6001))]).window(2000, [iv((1900, 2400, 7000, 7500))]),
        lambda s, f, o: s["frontier"] == 1 and s["nf"] == 3 and s["flags"] == 0)
    add("reach passes over a window that did not run",
        DM.Round().window(1000, [iv((900, 2501, 4900, 6501))]).window(2000, [iv(HIT)], act=False).window(2500, [iv((2400, 2900, 7000, 7500))]),
        lambda s, f, o: s["frontier"] == 1)
    for at in (0, 1, None):
        for how in ("window wide", "found wide", "roll wide", "bad window", "hit wide"):
            R = DM.Round()
            for j in range(3):
                loc, hit = 1000 * (j + 1), (1000 * (j + 1) - 100, 1000 * (j + 1) + 300, 4900, 5300)
                if j != at:
                    R.window(loc, [iv(hit), iv(hit, ref=(9000, 9100), hflags=2, rflags=1)])  # (completed WIDE records are records)
                elif how in ("window wide", "found wide"):
                    R.window(loc, [iv(hit)], flags=4 if how == "window wide" else 8)
                elif how in ("roll wide", "bad window"):
                    R.window(loc, [iv(hit), iv(None, ref=(0, 0), jaccard=0, rflags=1 if how == "roll wide" else 2, f1=8, hflags=1)])
                else:
                    R.window(loc, [iv(hit), iv(None, ref=(9000, 9100), hflags=2, f2=8)])
            want = 3 if at is None else at
            add("incomplete (%s) at %s" % (how, at), R,
                lambda s, f, o, want=want: s["frontier"] == want and s["flags"] == (DM.INCOMPLETE if want < 3 else 0) and s["nf"] == 2 + 2 * want)
    # capacities: the round adds 3 records to found and 2 to out
    three = DM.Round().window(1000, [iv(HIT), iv((900, 1200, 4900, 5300), ref=(9000, 9100))]).window(3000, [iv((2900, 3300, 4900, 5300))])
    add("found capacity exact", three, lambda s, f, o: s["flags"] == 0 and s["nf"] == 5 and s["n_out"] == 3, found_cap=5, out_cap=3)
    add("found capacity one short", three, lambda s, f, o: s["flags"] == DM.OVERFLOW and (s["nf"], s["need_found"], s["frontier"]) == (2, 5, 0),
        found_cap=4, out_cap=3)
    add("out capacity one short", three, lambda s, f, o: s["flags"] == DM.OVERFLOW and (s["n_out"], s["need_out"], s["attempted"]) == (1, 3, 0),
        found_cap=5, out_cap=2)
    return out


def big_rounds():
    """Rounds at the sizes where the device form takes another path: more kept records than lanes, the cap, many windows."""
    out = []
    rng = np.random.default_rng(3)

    def many(n):  # n kept hits in one window, none overlapped by another; every third repeats the one before
        ivs = []
        for t in range(n):
            u = t - 1 if t % 3 == 2 else t
            ivs.append(iv((900 - u % 7, 1300 + u, 10000 + 1000 * u, 10400 + 1000 * u), ref=(100 + t, 200 + t), hj=t))
        return ivs
    out.append(("65 candidates", DM.Round().window(1000, many(65)).window(5000, [iv((4900, 5300, 1, 400))]), [], [], None, None, 0,
                lambda s, f, o: s["frontier"] == 2 and s["nf"] == 66))
    out.append(("the cap exactly", DM.Round().window(1000, many(DM.MAX_KEPT)), [], [], None, None, 0,
                lambda s, f, o: s["frontier"] == 1 and s["nf"] == DM.MAX_KEPT))
    out.append(("one kept hit more than the cap", DM.Round().window(500, [iv((400, 900, 1, 400))]).window(1000, many(DM.MAX_KEPT + 1)), [], [], None,
                None, 0, lambda s, f, o: s["frontier"] == 1 and s["flags"] == DM.INCOMPLETE and s["nf"] == 1))
    out.append(("a round of one window", DM.Round().window(1000, [iv(HIT)]), [], [], None, None, 7, lambda s, f, o: s["frontier"] == 1 and o == [(7,) + HIT + (7,)]))
    for n, stop in ((300, None), (300, 170), (2100, 2050), (2100, None)):
        R = DM.Round()
        for j in range(n):
            loc = 1000 + 50 * j
            ivs = []
            for t in range(int(rng.integers(0, 4))):
                end = loc + (51 if j + 1 == stop and t == 0 else int(rng.choice([30, 50])))
                ivs.append(iv((loc - 10 - t, end, 7000 + 200 * t, 7100 + 200 * t), ref=(100 * t, 100 * t + 100), jaccard=int(rng.integers(-1, 5)),
                              verdict=int(rng.random() < 0.1), f2=2 if rng.random() < 0.1 else 0))
            if j + 1 == stop:
                ivs = [iv((loc - 10, loc + 51, 7000, 7100), ref=(0, 100))] + ivs
            R.window(loc, ivs, act=rng.random() < 0.9 or j + 1 == stop or j == stop)
        want = len(R.act) if stop is None else R.act.index(stop)
        out.append(("a round of %d windows, stopped at %s" % (n, stop), R, [(1, 2, 3, 4)], [], None, None, 0,
                    lambda s, f, o, want=want: s["frontier"] == want and s["flags"] == 0))
    return out


def check_accept(call, case, extz2):
    """One case through `call` (search_accept_host, or an engine's search_accept_raw) against the model."""
    name, R, found, outs, found_cap, out_cap, base, shows = case
    A = R.arrays(extz2)
    n = len(A["rolls"])
    found_cap = len(found) + n if found_cap is None else found_cap
    out_cap = len(outs) + n if out_cap is None else out_cap
    status, want_found, want_out = DM.accept(A, found, outs, found_cap, out_cap, window_base=base)
    assert shows(status, want_found, want_out), (name, status)
    out_in = np.zeros(len(outs), extz2.SEARCH_PAIR_HIT_DTYPE)
    for k, row in enumerate(outs):
        out_in[k] = row
    rc, got, found_buf, out_buf = call(A["q"], A["act"], A["windows"], A["first"], A["rolls"], A["overlap"], A["filt"], A["hits"],
                                       A["hit_filter"], A["init_len"], A["min_read_size"], FM.found_records(found), out_in,
                                       found_cap=found_cap, out_cap=out_cap, window_base=base)
    assert rc == 0, name
    assert {f: int(got[f]) for f in got.dtype.names} == status, name
    assert FM.rows_of(found_buf[:status["nf"]]) == [tuple(r) for r in want_found], name
    assert [tuple(int(x) for x in r) for r in out_buf[:status["n_out"]].tolist()] == [tuple(r) for r in want_out], name
    # nothing behind the new counts was written, the canaries behind the capacities included
    assert set(found_buf[status["nf"]:].tobytes()) <= {0xEE} and set(out_buf[status["n_out"]:].tobytes()) <= {0xEE}, name
    return got, found_buf, out_buf


def test_accept_host_is_the_model_on_hand_made_rounds():
    extz2 = ex()
    cases = hand_made_rounds()
    assert len(cases) > 30
    for case in cases:
        check_accept(extz2.search_accept_host, case, extz2)


def test_accept_host_is_the_model_at_the_device_forms_sizes():
    extz2 = ex()
    for case in big_rounds():
        check_accept(extz2.search_accept_host, case, extz2)


def test_accept_host_with_records_beyond_n_max():
    """A window whose records lie beyond n_max is incomplete: the frontier stops there."""
    extz2 = ex()
    R = DM.Round().window(1000, [iv(HIT)]).window(3000, [iv((2900, 3300, 4900, 5300))])
    A = R.arrays(extz2)
    status, want_found, _ = DM.accept(A, [], [], 2, 2, n_max=1)
    assert (status["frontier"], status["flags"], status["nf"]) == (1, DM.INCOMPLETE, 1)
    rc, got, found_buf, _ = extz2.search_accept_host(A["q"], A["act"], A["windows"], A["first"], A["rolls"], A["overlap"], A["filt"], A["hits"],
                                                     A["hit_filter"], 100, 100, FM.found_records([]), np.zeros(0, extz2.SEARCH_PAIR_HIT_DTYPE),
                                                     found_cap=2, out_cap=2, n_max=1)
    assert rc == 0 and {f: int(got[f]) for f in got.dtype.names} == status and FM.rows_of(found_buf[:1]) == [HIT]


# ---- 3. refusals, names, sizes ----

def test_accept_refusals():
    extz2 = ex()
    A = DM.Round().window(1000, [iv(HIT)]).window(2000, [iv(HIT)]).arrays(extz2)
    none = np.zeros(0, extz2.SEARCH_PAIR_HIT_DTYPE)

    def code(found=FM.found_records([]), out=none, **change):
        a = dict(A, **{k: v for k, v in change.items() if k in A})
        kw = {k: v for k, v in change.items() if k not in A}
        return extz2.search_accept_host(a["q"], a["act"], a["windows"], a["first"], a["rolls"], a["overlap"], a["filt"], a["hits"],
                                        a["hit_filter"], a["init_len"], a["min_read_size"], found, out, **kw)[0]
    assert code() == 0
    assert code(init_len=0) == SDF_ERR_INVALID and code(init_len=(1 << 30) + 1) == SDF_ERR_UNSUPPORTED
    assert code(min_read_size=-1) == SDF_ERR_INVALID and code(reserved=1) == SDF_ERR_UNSUPPORTED
    assert code(act=np.array([1, 0], np.uint32)) == SDF_ERR_INVALID and code(act=np.array([0, 0], np.uint32)) == SDF_ERR_INVALID
    assert code(act=np.array([0, 2], np.uint32)) == SDF_ERR_INVALID
    assert code(first=np.array([0, 2, 1], np.uint64)) == SDF_ERR_INVALID and code(first=np.array([1, 1, 2], np.uint64)) == SDF_ERR_INVALID
    assert code(found=FM.found_records([HIT, HIT]), found_cap=1) == SDF_ERR_INVALID  # nf > found_cap
    lib = extz2.load_library()
    status = np.zeros(1, extz2.ACCEPT_STATUS_DTYPE)
    R = extz2.accept_round(None, 0, None, 0, None, None, 0, None, None, None, None, None, 100, 100)
    assert lib.sdf_search_accept_host(C.byref(R), None, 0, 0, None, 0, 0, status.ctypes.data) == 0 and status["frontier"][0] == 0
    assert lib.sdf_search_accept_host(None, None, 0, 0, None, 0, 0, status.ctypes.data) == SDF_ERR_INVALID
    assert lib.sdf_search_accept_host(C.byref(R), None, 0, 0, None, 0, 0, None) == SDF_ERR_INVALID
    assert lib.sdf_search_accept_host(C.byref(R), None, 0, 1, None, 0, 0, status.ctypes.data) == SDF_ERR_INVALID  # a capacity without a buffer
    assert lib.sdf_search_accept_host(C.byref(R), None, 0, 0, None, 0, 1 << 31, status.ctypes.data) == SDF_ERR_INVALID
    one = extz2.accept_round(None, 1, None, 1, None, None, 0, None, None, None, None, None, 100, 100)
    assert lib.sdf_search_accept_host(C.byref(one), None, 0, 0, None, 0, 0, status.ctypes.data) == SDF_ERR_INVALID  # a round without arrays


def test_pair_host_refusals():
    I = DM.inputs(*INPUTS[0])

    def code(**change):
        i = dict(I, **{k: v for k, v in change.items() if k in I})
        return host_pair(i, **{k: v for k, v in change.items() if k not in I})[0]
    assert code(k=0) == SDF_ERR_UNSUPPORTED and code(k=16) == SDF_ERR_UNSUPPORTED
    assert code(w=0) == SDF_ERR_UNSUPPORTED and code(w=1001) == SDF_ERR_UNSUPPORTED
    assert code(init_len=0) == SDF_ERR_INVALID
    assert code(limit=[0, 1, 0]) == SDF_ERR_UNSUPPORTED
    assert code(q_range=(-1, 100, 0)) == SDF_ERR_INVALID and code(q_range=(0, -1, 0)) == SDF_ERR_INVALID
    assert code(r_range=(len(I["pool"]) - 10, 11, 0)) == SDF_ERR_INVALID
    assert code(r_range=I["r_range"][:2] + (2,)) == SDF_ERR_UNSUPPORTED
    assert code(same_genome=1) == SDF_ERR_INVALID  # different ranges
    assert code(same_genome=1, r_range=I["q_range"][:2] + (1,)) == SDF_ERR_INVALID  # a strand flag
    assert code(extend=ex().extend_params(max_error=0.1, max_edit_error=0.1)) == SDF_ERR_INVALID
    assert code(filter=ex().filter_params(reserved=1)) == SDF_ERR_UNSUPPORTED


def test_library_exports_the_entry_points_and_record_sizes():
    extz2 = ex()
    lib = extz2.load_library()
    for name in ("sdf_search_accept", "sdf_search_accept_device", "sdf_search_accept_host", "sdf_search_pair_host"):
        assert hasattr(lib, name), name
    assert extz2.SEARCH_PAIR_HIT_DTYPE.itemsize == 24 and extz2.ACCEPT_STATUS_DTYPE.itemsize == 64 and extz2.PAIR_STATS_DTYPE.itemsize == 56
    assert (extz2.ACCEPT_MAX_KEPT, extz2.ACCEPT_INCOMPLETE, extz2.ACCEPT_OVERFLOW) == (DM.MAX_KEPT, DM.INCOMPLETE, DM.OVERFLOW)
    assert extz2.ACCEPT_MAX_KEPT >= 64
    assert C.sizeof(extz2._AcceptRound) == 112 and C.sizeof(extz2._PairParams) == 120
