"""CPU side of the traceback tests: tests/tbgen.py's designed CIGARs against the CPU oracle, and the planner's routing of
the shapes tests/test_gpu_traceback.py runs.

The design -- [head M, L gap, tail M] and its kin -- is asserted on the oracle's output with NO allowance: a case that misses
it would test something else than it says (a run at the group size), so the input is changed, never the assertion.  The
families that are oracle-compared only (band edge, trailing gap, max-cell start) carry no design (`Case.runs is None`)."""
import ctypes as C

import numpy as np
import pytest

import tbgen


def _words(oracle, c):
    return oracle.extz2(c.q, c.t, w=c.w, zdrop=c.zdrop, flag=c.flag)["cigar"].tolist()


def _designed(c):
    w = c.designed_words()
    return w[::-1] if c.flag & tbgen.REV_CIGAR else w


@pytest.mark.parametrize("G", tbgen.GROUPS)
def test_interior_gaps_have_the_designed_runs(oracle, G):
    """Family 1: 280 cases -- L in {G-1, G, G+1, 2G-1, 2G, 2G+1, 3G+5}, head in {G-1, G, G+1, 2G, 2G+1}, tail = head + 3, both
    sides, w = -1 and L + 8."""
    rng = np.random.default_rng(100 + G)
    cases = tbgen.family1(rng, G)
    assert len(cases) == 140 and all(c.runs for c in cases)
    missed = [c.tag for c in cases if _words(oracle, c) != _designed(c)]
    assert not missed, missed
    lens = {c.runs[1][1] for c in cases}
    assert lens == set(tbgen.edge_lengths(G))
    assert {c.runs[1][0] for c in cases} == {tbgen.INS, tbgen.DEL}


def test_leading_gaps_diagonals_and_many_runs_have_the_designed_runs(oracle):
    """Families 3 (leading form), 4 and 5, full band and banded as the routes take them."""
    rng = np.random.default_rng(7)
    cases = tbgen.family3(rng) + tbgen.family3(rng, band=8)
    for G in tbgen.GROUPS:
        cases += tbgen.family4(rng, G) + tbgen.family4(rng, G, w=7)
    cases += tbgen.family5(rng) + tbgen.family5(rng, w=16) + tbgen.family5(rng, w=64, counts=(65, 131))
    designed = [c for c in cases if c.runs is not None]
    assert len(designed) >= 24 + 40 + 20
    missed = [c.tag for c in designed if _words(oracle, c) != _designed(c)]
    assert not missed, missed
    assert {len(c.runs) for c in designed if c.family == 5} == {63, 65, 129, 131}
    # the CIGAR of 64 words (not design-asserted: a leading gap) has 64 words
    for f in (0, tbgen.REV_CIGAR):
        assert len(_words(oracle, tbgen.family5_even(rng, 64, f))) == 64


@pytest.mark.parametrize("route, G", tbgen.CALLS)
def test_every_designed_case_of_a_route_has_its_runs(oracle, route, G):
    """The shapes the GPU tests run (tbgen.route_cases): every case that carries a design has the designed runs."""
    cases = tbgen.route_cases(route, G)
    missed = [c.tag for c in cases if c.runs is not None and _words(oracle, c) != _designed(c)]
    assert not missed, missed
    assert sum(c.runs is not None for c in cases) >= len(cases) // 3
    # gap runs at the group's edges are in every route's list
    gaps = {ln for c in cases if c.runs for op, ln in c.runs if op != tbgen.M}
    assert {G - 1, G, G + 1} <= gaps, sorted(gaps)


def _plan(tasks, want, lds=160 * 1024):
    import sedef_amd
    from sedef_amd import extz2
    lib = sedef_amd.load_library()
    sc = extz2._scoring(extz2.sedef_mat(), 40, 1)
    n = len(tasks)
    per_task = np.zeros((n, 7), np.int64)
    per_chunk = np.zeros((64, 5), np.int64)
    nch = C.c_size_t(0)
    lib.sdf_debug_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_size_t, C.c_int, C.c_int, C.c_void_p,
                                   C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    rc = lib.sdf_debug_plan(C.byref(sc), tasks.ctypes.data, n, want, 64 << 30, lds, 0, per_task.ctypes.data,
                            per_chunk.ctypes.data, 64, C.byref(nch))
    return rc, per_task, per_chunk[:nch.value]


@pytest.mark.parametrize("route, G", [c for c in tbgen.CALLS if c[0] != "lane"])
def test_route_cases_plan_to_the_intended_kernel(monkeypatch, route, G):
    """sdf_debug_plan with the route's settings in the environment: every task of the call the GPU test makes is planned to
    the route's TaskKind and nreg, i.e. to the direction-flag layout the test means to walk.  (The lane kernel is planned on
    the device: not here.)"""
    R = tbgen.ROUTES[route]
    for k, v in R["settings"].items():
        monkeypatch.setenv(k, str(v))
    cases, copies, tasks, _ = tbgen.call_tasks(route, G)
    rc, pt, pc = _plan(tasks, R["want"])
    assert rc == 0
    assert (pt[:, 0] >= 0).all()
    kinds, nreg = pt[:, 3], pt[:, 2]
    off = np.flatnonzero(~np.isin(kinds, R["kinds"]) | ((nreg != R["nreg"]) if R["nreg"] is not None else (nreg <= 0)))
    assert len(off) == 0, [(cases[k % len(cases)].tag, int(kinds[k]), int(nreg[k])) for k in off[:6]]
    lay = {tbgen.layout_of(int(a), int(b)) for a, b in zip(kinds, nreg)}
    assert lay == {R["layout"]}
    if route in ("strip4", "strip8"):
        assert (nreg[kinds == tbgen.K_STRIP] == 8).all() and (nreg[kinds == tbgen.K_CHAIN] == int(route[5:])).all()
        # the three record forms: one wavefront (strip kernel), chains, and a task that has its wavefront to itself
        assert {tbgen.K_STRIP, tbgen.K_CHAIN} <= set(kinds.tolist())
        alone = np.flatnonzero((kinds == tbgen.K_STRIP) & (pt[:, 6] == np.arange(len(pt))))
        assert len(alone) >= 1
    if route == "pair_mixed":
        assert ((pt[:, 1] >= 130) & (pt[:, 1] < 140)).any()  # the MIXED flavour's launch classes
    if route == "pair":
        assert ((pt[:, 1] >= 120) & (pt[:, 1] < 130)).any()  # the TRACK flavour's (bands that run out)
