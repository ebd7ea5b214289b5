"""The resident search index on the device: sdf_search_index_build / _free / _info and sdf_search_pair_indexed
(sedef_amd/csrc/sdf_driver_api.hip).

Expected values: sdf_search_pair on the same ranges and parameters -- out, used and the three counters byte for byte -- and,
so that no comparison is empty against empty, sdf_search_pair_host on the same characters, which must report a hit in every
case (the seeds were chosen on the CPU for that, and the tests assert it)."""
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


def rng_of(i, rc=False):
    return (OFF[i], LENS[i], 1 if rc else 0)


def ex():
    from sedef_amd import extz2
    return extz2


@pytest.fixture(scope="module")
def eng():
    import sedef_amd
    e = sedef_amd.Extz2Engine(0)
    e.pool_upload(POOL)
    e.pool_sync()
    yield e
    e.close()


_handles, _hosted = {}, {}


def handle(eng, i, rc=False):
    if (i, rc) not in _handles:
        code, h = eng.search_index_build(rng_of(i, rc), k=12, w=16)
        assert code == 0 and h
        _handles[(i, rc)] = h
    return _handles[(i, rc)]


def host_hits(q, r, r_rc, same):
    """sdf_search_pair_host on the pool's characters: the hits of the case (at least one)."""
    key = (q, r, r_rc, same)
    if key not in _hosted:
        code, hits, used, _ = ex().search_pair_host(POOL, rng_of(q), rng_of(r, r_rc), same_genome=same,
                                                    extend=ex().extend_params(same_genome=same), **KW)
        assert code == 0 and used >= 1, key
        _hosted[key] = hits
    return _hosted[key]


def same_call(eng, q, r, r_rc=False, same=False, **more):
    """sdf_search_pair_indexed on the handles equals sdf_search_pair on their ranges, and both the host form's hits."""
    kw = dict(KW, same_genome=same, extend=ex().extend_params(same_genome=same), **more)
    want = eng.search_pair(rng_of(q), rng_of(r, r_rc), **kw)
    got = eng.search_pair_indexed(handle(eng, q), handle(eng, r, r_rc), **kw)
    assert want[0] == 0 and got[0] == 0
    assert got[2] == want[2] >= 1 and got[1].tobytes() == want[1].tobytes()
    assert got[1].tobytes() == host_hits(q, r, r_rc, same).tobytes()
    for f in COUNTERS:
        assert int(got[3][f]) == int(want[3][f]), f
    return got


@pytest.mark.parametrize("round_windows", (1, 3, 64))
def test_two_ranges_for_every_round_size(eng, round_windows):
    same_call(eng, 0, 1, round_windows=round_windows)


@pytest.mark.parametrize("round_windows", (1, 3, 64))
def test_same_genome_is_one_handle_on_both_sides(eng, round_windows):
    same_call(eng, 0, 0, same=True, round_windows=round_windows)


def test_a_reverse_complemented_reference(eng):
    """The inverted copy: nothing on the forward strand, a hit on the other."""
    code, hits, used, _ = ex().search_pair_host(POOL, rng_of(0), rng_of(3), **KW)
    assert code == 0 and used == 0
    same_call(eng, 0, 3, r_rc=True)
    got = eng.search_pair_indexed(handle(eng, 0), handle(eng, 3), **KW)
    assert got[0] == 0 and got[2] == 0


def test_one_handle_as_query_twice_then_as_reference_and_a_pair_twice(eng):
    builds = eng.search_index_builds()[0]
    a = same_call(eng, 0, 1)
    same_call(eng, 0, 3, r_rc=True)
    same_call(eng, 1, 0)  # the first record's handle as the reference now
    same_call(eng, 0, 0, same=False)  # ... and as both sides without same_genome
    b = same_call(eng, 0, 1)  # the first pair again: the calls between left the handles as they were
    assert a[1].tobytes() == b[1].tobytes()
    # every handle was built once (the cache of this module), whatever the number of calls
    assert eng.search_index_builds()[0] - builds <= 3


def test_a_pair_that_takes_the_host_step(eng):
    got = same_call(eng, 0, 1, debug_host_every=2)
    assert int(got[3]["windows_host"]) >= 1


def test_info_names_what_was_built(eng):
    d = eng.search_index_info(handle(eng, 3, True))
    assert (int(d["off"]), int(d["len"]), int(d["flags"])) == rng_of(3, True)
    assert (int(d["k"]), int(d["w"]), int(d["separate_lowercase"]), int(d["stale"])) == (12, 16, 1, 0)
    # the counts and the threshold are those of the two calls the build makes
    first, _, n_groups, threshold = eng.pool_minimizer_index([rng_of(3)[:2]], k=12, w=16, rc=[True])
    assert int(d["n_minimizers"]) == int(d["n_sorted"]) == int(first[1]) >= 1
    assert int(d["threshold"]) == int(threshold[0]) == 1 << 31 and int(d["n_groups"]) == int(n_groups[0])
    assert int(d["device_bytes"]) >= 32 * int(d["n_minimizers"])


def test_a_handle_freed_and_rebuilt(eng):
    handle(eng, 1)
    live = eng.search_index_builds()[1]
    code, h = eng.search_index_build(rng_of(2), k=12, w=16)
    assert code == 0 and eng.search_index_builds()[1] == live + 1
    want = eng.search_pair(rng_of(1), rng_of(2), **KW)
    assert want[0] == 0 and want[1].tobytes() == host_hits(1, 2, False, False).tobytes()  # (the host form: at least one hit)
    got = eng.search_pair_indexed(handle(eng, 1), h, **KW)
    assert got[0] == 0 and got[1].tobytes() == want[1].tobytes()
    assert eng.search_index_free(h) == 0 and eng.search_index_builds()[1] == live
    assert eng.search_index_free(h) == -4  # (no longer a handle of this context: refused, not read)
    assert eng.search_pair_indexed(handle(eng, 1), h, **KW)[0] == -4
    code, h2 = eng.search_index_build(rng_of(2), k=12, w=16)
    assert code == 0
    again = eng.search_pair_indexed(handle(eng, 1), h2, **KW)
    assert again[0] == 0 and again[1].tobytes() == want[1].tobytes()
    assert eng.search_index_free(h2) == 0 and eng.search_index_free(None) == 0


def test_two_contexts_share_a_pool_each_with_its_own_handles(eng):
    import sedef_amd
    other = sedef_amd.Extz2Engine(0)
    try:
        other.pool_share(eng)
        code, oq = other.search_index_build(rng_of(0), k=12, w=16)
        code2, orr = other.search_index_build(rng_of(1), k=12, w=16)
        assert code == 0 and code2 == 0
        want = eng.search_pair_indexed(handle(eng, 0), handle(eng, 1), **KW)
        got = other.search_pair_indexed(oq, orr, **KW)
        assert got[0] == 0 and want[0] == 0 and got[1].tobytes() == want[1].tobytes()
        assert got[1].tobytes() == host_hits(0, 1, False, False).tobytes()  # (the host form: at least one hit)
        # a handle is its own context's alone
        assert other.search_pair_indexed(handle(eng, 0), orr, **KW)[0] == -4
        assert eng.search_pair_indexed(oq, handle(eng, 1), **KW)[0] == -4
        assert other.search_index_builds() == (2, 2)
    finally:
        other.close()  # (with both handles live: they go with their context)
    again = eng.search_pair_indexed(handle(eng, 0), handle(eng, 1), **KW)
    assert again[0] == 0 and again[1].tobytes() == want[1].tobytes()


def test_refusals_precede_the_first_launch_and_leave_the_context_usable(eng):
    q, r, q_rc = handle(eng, 0), handle(eng, 1), handle(eng, 0, True)
    before = eng.last_launches()

    def code(qh=q, rh=r, **kw):
        return eng.search_pair_indexed(qh, rh, **dict(KW, **kw))[0]
    assert code(qh=None) == -4 and code(rh=None) == -4
    assert code(k=11) == -4 and code(w=15) == -4 and code(separate_lowercase=False) == -4
    assert code(same_genome=True) == -4  # two handles
    assert code(qh=q, rh=q_rc, same_genome=True) == -4  # ... even of one range, on the other strand
    assert code(min_read_size=0) == -4 and code(limit=[0, 1, 0]) == -3  # (sdf_search_pair's own, with their codes)
    assert eng.search_index_build((OFF[-1], 1, 0))[0] == -4 and eng.search_index_build(rng_of(0), k=16)[0] == -3
    assert eng.search_index_build(rng_of(0), w=0)[0] == -4 and eng.search_index_build(rng_of(0)[:2] + (2,))[0] == -3
    assert eng.last_launches() == before
    same_call(eng, 0, 1)


def test_a_replaced_pool_makes_the_handles_stale():
    """(an engine of its own: the module's pool stays)"""
    import sedef_amd
    e = sedef_amd.Extz2Engine(0)
    try:
        e.pool_upload(POOL)
        e.pool_sync()
        code, h = e.search_index_build(rng_of(0), k=12, w=16)
        got = e.search_pair_indexed(h, h, same_genome=True, extend=ex().extend_params(same_genome=True), **KW)
        assert code == 0 and got[0] == 0 and got[1].tobytes() == host_hits(0, 0, False, True).tobytes()  # (at least one hit)
        e.pool_upload(POOL)
        e.pool_sync()
        assert int(e.search_index_info(h)["stale"]) == 1
        assert e.search_pair_indexed(h, h, same_genome=True, extend=ex().extend_params(same_genome=True), **KW)[0] == -4
        assert e.search_index_free(h) == 0
    finally:
        e.close()
