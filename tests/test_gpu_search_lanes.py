"""Several pairs in flight on one GPU: sdf_search_lanes_open / _close and sdf_search_pairs_indexed
(sedef_amd/csrc/sdf_lanes_api.hip).

Expected values: sdf_search_pair_indexed (sdf_search_pair_indexed_wide where n_wide_max is given) on the owner, one job after the
other -- every slice of the batch equals that call's hits byte for byte, and the four counters agree.  The pool, the table and
the records are those of tests/test_gpu_search_index.py, where every pair kind is shown to report what the host form reports;
one batch holds them all, and the tests assert that at least five of its jobs have hits and at least one has none."""
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (at collection: before the library brings a HIP runtime of its own along)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import search_cmd_gen as G  # noqa: E402

pytestmark = pytest.mark.gpu

# four records of 5-12 kb: a copy inside the first, one from the first in the second, one from the second in the third, and an
# INVERTED copy of the first's end in the fourth; lowercase stretches and an N run
LENS = [12000, 9000, 7000, 5000]
COPIES = [(0, 500, 2500, 0, 7000, 0.05, False), (0, 3500, 2000, 1, 1000, 0.04, False), (1, 5000, 1800, 2, 3000, 0.08, False),
          (0, 9800, 1600, 3, 2000, 0.03, True)]
RECS = G.records(5, LENS, COPIES, lower=[(0, 2000, 300), (1, 1200, 200), (3, 100, 400)], n_runs=[(2, 6000, 150)])
POOL = b"".join(RECS)
OFF = np.concatenate([[0], np.cumsum(LENS)]).tolist()
LIMIT = [0] + [1] * 4095  # (what `sedef search` computes at the default errors: DESIGN.md)
KW = dict(k=12, w=16, min_read_size=700, limit=LIMIT)
COUNTERS = ("attempted", "jaccard_failed", "interval_failed", "windows_scheduled")
INVALID, UNSUPPORTED, OVERFLOW = -4, -3, -5

# (query, reference, reference reverse-complemented, same_genome): the 16 ordered forward pairs, each record against itself
# with same_genome, the inverted copy on the other strand, and one pair twice more
PAIRS = [(q, r, False, False) for r in range(4) for q in range(4)] + [(i, i, False, True) for i in range(4)] + \
    [(0, 3, True, False)] + [(0, 1, False, False)] * 2


def rng_of(i, rc=False):
    return (OFF[i], LENS[i], 1 if rc else 0)


def ex():
    from sedef_amd import extz2
    return extz2


def new_engine():
    import sedef_amd
    e = sedef_amd.Extz2Engine(0)
    e.pool_upload(POOL)
    e.pool_sync()
    return e


def build_handles(e):
    h = {}
    for i in range(4):
        for rc in ((False, True) if i == 3 else (False,)):
            code, h[(i, rc)] = e.search_index_build(rng_of(i, rc), k=12, w=16)
            assert code == 0 and h[(i, rc)]
    return h


@pytest.fixture(scope="module")
def eng():
    e = new_engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def handles(eng):
    return build_handles(eng)


def jobs_of(h, pairs=PAIRS):
    return [(h[(q, False)], h[(r, r_rc)], same) for q, r, r_rc, same in pairs]


_single = {}


def single(eng, h, pair, n_wide_max=0, **more):
    """The owner's single-pair call of one job, computed once per (job, configuration)."""
    key = (pair, n_wide_max, tuple(sorted(more.items())))
    if key not in _single:
        q, r, r_rc, same = pair
        kw = dict(KW, same_genome=same, extend=ex().extend_params(same_genome=same), **more)
        got = (eng.search_pair_indexed_wide(h[(q, False)], h[(r, r_rc)], n_wide_max, **kw) if n_wide_max
               else eng.search_pair_indexed(h[(q, False)], h[(r, r_rc)], **kw))
        assert got[0] == 0, key
        _single[key] = got
    return _single[key]


def check_batch(eng, h, got, pairs=PAIRS, n_wide_max=0, **more):
    """Every slice equals the single-pair call; the four counters; first[] as the header states it.  Returns the jobs with hits."""
    code, hits, first, stats = got
    assert code == 0
    assert int(first[0]) == 0 and np.all(np.diff(first.astype(np.int64)) >= 0) and int(first[-1]) == len(hits)
    with_hits = 0
    for j, pair in enumerate(pairs):
        want = single(eng, h, pair, n_wide_max, **more)
        mine = hits[int(first[j]):int(first[j + 1])]
        assert len(mine) == want[2] and mine.tobytes() == want[1].tobytes(), (j, pair)
        for f in COUNTERS:
            assert int(stats[j][f]) == int(want[3][f]), (j, pair, f)
        with_hits += len(mine) > 0
    return with_hits


def with_lanes(eng, n, body):
    code, lanes = eng.search_lanes_open(n)
    assert code == 0 and lanes
    try:
        return body(lanes)
    finally:
        assert eng.search_lanes_close(lanes) == 0


@pytest.mark.parametrize("round_windows", (1, 64))
@pytest.mark.parametrize("n_lanes", (1, 2, 4, 16))
def test_every_slice_is_the_single_pair_call(eng, handles, n_lanes, round_windows):
    got = with_lanes(eng, n_lanes, lambda lanes: eng.search_pairs_indexed(lanes, jobs_of(handles), round_windows=round_windows, **KW))
    with_hits = check_batch(eng, handles, got, round_windows=round_windows)
    assert with_hits >= 5 and with_hits < len(PAIRS)  # (no comparison of nothing with nothing, and a job without a hit)
    # the pair that is there three times has three equal slices
    first, hits = got[2], got[1]
    same = [hits[int(first[j]):int(first[j + 1])].tobytes() for j, p in enumerate(PAIRS) if p == (0, 1, False, False)]
    assert len(same) == 3 and len(set(same)) == 1 and same[0]


def test_with_the_wide_windows_on_the_device(eng, handles):
    got = with_lanes(eng, 4, lambda lanes: eng.search_pairs_indexed(lanes, jobs_of(handles), n_wide_max=64, **KW))
    assert check_batch(eng, handles, got, n_wide_max=64) >= 5


def test_the_host_step_and_its_pool_fetch_on_views_in_parallel(eng, handles):
    got = with_lanes(eng, 4, lambda lanes: eng.search_pairs_indexed(lanes, jobs_of(handles), debug_host_every=2, **KW))
    assert check_batch(eng, handles, got, debug_host_every=2) >= 5
    # (every second scheduled window is the host's: a job with two scheduled windows took the host step)
    assert all(int(s["windows_host"]) >= 1 for s in got[3] if int(s["windows_scheduled"]) >= 2)
    assert sum(int(s["windows_scheduled"]) >= 2 for s in got[3]) >= 5


def test_no_job_and_fewer_jobs_than_lanes(eng, handles):
    def body(lanes):
        code, hits, first, stats = eng.search_pairs_indexed(lanes, [], **KW)
        assert code == 0 and len(hits) == 0 and first.tolist() == [0] and len(stats) == 0
        two = [(0, 1, False, False), (1, 2, False, False)]
        assert check_batch(eng, handles, eng.search_pairs_indexed(lanes, jobs_of(handles, two), **KW), pairs=two) == 2
    with_lanes(eng, 4, body)


def test_a_short_cap_reports_the_need_and_a_second_call_succeeds(eng, handles):
    jobs = jobs_of(handles, PAIRS[:6] + PAIRS[16:18])  # (hits in (0, 0), (0, 1) and the two same_genome jobs at least)

    def body(lanes):
        full = eng.search_pairs_indexed(lanes, jobs, **KW)
        need = int(full[2][-1])
        assert full[0] == 0 and need >= 3
        code, hits, first, _ = eng.search_pairs_indexed(lanes, jobs, cap=need - 1, **KW)
        assert code == OVERFLOW and len(hits) == 0 and first.tolist() == full[2].tolist()
        code, hits, first, _ = eng.search_pairs_indexed(lanes, jobs, cap=0, **KW)
        assert code == OVERFLOW and first.tolist() == full[2].tolist()
        again = eng.search_pairs_indexed(lanes, jobs, cap=need, **KW)
        assert again[0] == 0 and again[1].tobytes() == full[1].tobytes() and again[2].tolist() == full[2].tolist()
    with_lanes(eng, 4, body)


def test_refusals_precede_the_first_launch_and_leave_the_context_usable(eng, handles):
    good = jobs_of(handles, PAIRS[:3])
    code, freed = eng.search_index_build(rng_of(2), k=12, w=16)
    assert code == 0 and eng.search_index_free(freed) == 0
    other = new_engine()
    try:
        code, foreign = other.search_index_build(rng_of(0), k=12, w=16)
        assert code == 0

        def body(lanes):
            before = eng.last_launches()

            def code_of(jobs=good, use=lanes, **kw):
                return eng.search_pairs_indexed(use, jobs, **dict(KW, **kw))[0]
            q, r = handles[(0, False)], handles[(1, False)]
            assert code_of(use=None) == INVALID  # a null pointer
            assert code_of(jobs=good + [(None, r, False)]) == INVALID and code_of(jobs=good + [(q, None, False)]) == INVALID
            assert b"job 3" in eng.lib.sdf_last_error(eng.ctx)
            assert code_of(jobs=good + [(freed, r, False)]) == INVALID and code_of(jobs=[(q, foreign, False)] + good) == INVALID
            assert b"job 0" in eng.lib.sdf_last_error(eng.ctx)
            assert code_of(k=11) == INVALID and code_of(w=15) == INVALID and code_of(separate_lowercase=False) == INVALID
            assert code_of(jobs=good + [(q, r, True)]) == INVALID  # same_genome with two handles
            assert code_of(jobs=good + [(handles[(3, False)], handles[(3, True)], True)]) == INVALID  # ... even of one range
            # then sdf_search_pair_indexed_wide's own, with their codes
            assert code_of(min_read_size=0) == INVALID and code_of(limit=[0, 1, 0]) == UNSUPPORTED
            assert eng.search_pairs_indexed(lanes, good, n_wide_max=(1 << 20) + 1, **KW)[0] == UNSUPPORTED
            # a handle refused in a later job comes before a range refused in an earlier one
            assert code_of(jobs=good + [(None, r, False)], limit=[0, 1, 0]) == INVALID
            # lanes of another engine
            assert other.search_pairs_indexed(lanes, [(foreign, foreign, True)], **KW)[0] == INVALID
            assert other.search_lanes_close(lanes) == INVALID
            assert eng.last_launches() == before
            check_batch(eng, handles, eng.search_pairs_indexed(lanes, good, **KW), pairs=PAIRS[:3])
            return lanes
        closed = with_lanes(eng, 2, body)
        # closed lanes; lanes outside 1 .. 16
        before = eng.last_launches()
        assert eng.search_pairs_indexed(closed, good, **KW)[0] == INVALID and eng.search_lanes_close(closed) == INVALID
        assert eng.search_lanes_close(None) == 0
        assert eng.search_lanes_open(0) == (INVALID, None) and eng.search_lanes_open(17) == (INVALID, None)
        assert eng.last_launches() == before
    finally:
        other.close()


def test_the_pool_rule_and_the_bytes_of_open_lanes():
    """(an engine of its own: the module's pool stays)"""
    from sedef_amd.extz2 import SdfError
    e = new_engine()
    try:
        h = build_handles(e)
        pairs = [(0, 1, False, False), (0, 0, False, True)]
        want = [e.search_pair_indexed(h[(q, False)], h[(r, r_rc)], same_genome=same, **KW) for q, r, r_rc, same in pairs]
        assert all(w[0] == 0 and w[2] >= 1 for w in want)
        line = RECS[1][:600]
        bytes0 = e.device_bytes()
        code, lanes = e.search_lanes_open(3)
        assert code == 0 and e.device_bytes() > bytes0
        got = e.search_pairs_indexed(lanes, jobs_of(h, pairs), **KW)
        assert got[0] == 0 and e.device_bytes() > bytes0
        with pytest.raises(SdfError, match="pool is shared"):
            e.pool_append_fasta(line + b"\n", 600, 600, 601)
        assert e.search_lanes_close(lanes) == 0 and e.device_bytes() == bytes0
        # after close the pool grows again, and the handles answer as before -- alone and through new lanes
        assert e.pool_append_fasta(line + b"\n", 600, 600, 601) == len(POOL)
        e.pool_sync()
        code, lanes = e.search_lanes_open(2)
        assert code == 0
        again = e.search_pairs_indexed(lanes, jobs_of(h, pairs), **KW)
        assert again[0] == 0 and again[1].tobytes() == got[1].tobytes() and again[2].tolist() == got[2].tolist()
        for j, (pair, w) in enumerate(zip(pairs, want)):
            now = e.search_pair_indexed(h[(pair[0], False)], h[(pair[1], pair[2])], same_genome=pair[3], **KW)
            assert now[0] == 0 and now[2] >= 1 and now[1].tobytes() == w[1].tobytes()
            assert got[1][int(got[2][j]):int(got[2][j + 1])].tobytes() == w[1].tobytes()
    finally:
        e.close()  # (with lanes still open: they go with their engine)
    # ... and a new engine works afterwards
    e2 = new_engine()
    try:
        h2 = build_handles(e2)
        code, lanes = e2.search_lanes_open(2)
        got = e2.search_pairs_indexed(lanes, jobs_of(h2, pairs), **KW)
        assert code == 0 and got[0] == 0 and int(got[2][-1]) >= 2
    finally:
        e2.close()


def test_a_stale_handle_in_a_later_job_is_refused_against_the_owners_pool():
    """A handle that outlived a pool replacement: checked against the OWNER's pool_epoch (a lane's own moved when it took its
    view), for every job before the first launch.  (an engine of its own: the module's pool stays)"""
    e = new_engine()
    try:
        code, old = e.search_index_build(rng_of(0), k=12, w=16)
        assert code == 0
        e.pool_upload(POOL)  # the pool replaced: `old` is stale from here on
        e.pool_sync()
        assert int(e.search_index_info(old)["stale"]) == 1
        h = build_handles(e)
        pairs = [(0, 1, False, False), (1, 2, False, False), (0, 0, False, True)]
        want = [e.search_pair_indexed(h[(q, False)], h[(r, r_rc)], same_genome=same, **KW) for q, r, r_rc, same in pairs]
        assert all(w[0] == 0 and w[2] >= 1 for w in want)
        code, lanes = e.search_lanes_open(2)
        assert code == 0
        good = jobs_of(h, pairs)
        before = e.last_launches()
        for bad in ((old, h[(1, False)], False), (h[(0, False)], old, False), (old, old, True)):
            got = e.search_pairs_indexed(lanes, good + [bad], **KW)
            assert got[0] == INVALID and len(got[1]) == 0
            text = e.lib.sdf_last_error(e.ctx)
            assert b"job 3" in text and b"replaced" in text
        assert e.last_launches() == before
        got = e.search_pairs_indexed(lanes, good, **KW)
        assert got[0] == 0 and e.last_launches() > before
        for j, w in enumerate(want):
            assert got[1][int(got[2][j]):int(got[2][j + 1])].tobytes() == w[1].tobytes()
            for f in COUNTERS:
                assert int(got[3][j][f]) == int(w[3][f])
        assert e.search_lanes_close(lanes) == 0 and e.search_index_free(old) == 0
    finally:
        e.close()
