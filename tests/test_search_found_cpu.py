"""Search against the SDs already found, host forms (sdf_search_windows_found_host, sdf_search_overlap_host): the exclusions of
the reference's search() and its is_overlap against an explicit list of found records.

Expected values: tests/found_model.py -- the record-list model (the header's definitions as brute force) and the point-level
model of the reference's ICL tree, which must agree with each other on a replay of windows in order -- and the reference's own
answers for an empty tree (tests/golden/search_windows_kat.json.gz).  Every comparison is exact."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import found_model as FM  # noqa: E402
import minim_model as M  # noqa: E402
import search_model as S  # noqa: E402
from test_search_windows_cpu import case_args, case_arrays, load_fixture, same_records  # noqa: E402

SDF_ERR_UNSUPPORTED, SDF_ERR_INVALID, SDF_ERR_OVERFLOW = -3, -4, -5
BIG = 1 << 31


def ex():
    from sedef_amd import extz2
    return extz2


def host_windows(q, r_sorted, found, visible, **kw):
    code, first, windows, out, used = ex().search_windows_found_host(q, r_sorted, found=found, visible=visible, **kw)
    assert code == 0 and used == int(first[-1]) == len(out)
    return first.astype(np.int64), windows, out


def host_overlap(q, first, rolls, found, visible_iv, init_len, min_read_size):
    code, out = ex().search_overlap_host(q, first, rolls, found, visible_iv, init_len, min_read_size)
    assert code == 0
    return out


# ---- 1. the empty list ----

def test_empty_list_is_the_plain_call_on_the_fixture():
    extz2 = ex()
    n_iv = 0
    for c in load_fixture()["cases"]:
        q, r = case_arrays(c)
        kw = case_args(c)
        code, first, windows, out, used = extz2.search_windows_host(q, r, **kw)
        assert code == 0
        plain = (first.astype(np.int64), windows, out)
        some = FM.found_records([(0, 10 ** 6, 0, 10 ** 6), (5, 900, 7, 1200)])
        for found, visible in ((FM.found_records([]), np.zeros(len(q), np.uint32)), (some, np.zeros(len(q), np.uint32))):
            same_records(host_windows(q, r, found, visible, **kw), plain)
        # ... and no interval overlaps anything: the roll's records are not needed for that, any record serves
        n = int(first[-1])
        rolls = np.zeros(n, extz2.SEARCH_ROLL_DTYPE)
        rolls["ref_start"], rolls["ref_end"] = out["start"], out["start"] + c["init_len"]
        for found, vis in ((FM.found_records([]), 0), (some, 0)):
            assert not host_overlap(q, first, rolls, found, np.full(n, vis, np.uint32), c["init_len"], c["init_len"]).any()
        n_iv += n
    assert n_iv > 100


# ---- 2. the replay: windows in order, the list and the point-level tree growing as hits pass ----

LETTERS = np.frombuffer(b"ACGT", np.uint8)


def draw_sequence(rng, unit, copies, gap):
    """Repeated blocks: `copies` mutated copies of `unit`, now and then two in tandem, with random stretches between them."""
    parts = []
    for c in range(copies):
        u = unit.copy()
        hit = rng.random(len(u)) < 0.03
        u[hit] = (u[hit] + 1) % 4
        if c == 0 or rng.random() < 0.5:
            parts.append(rng.integers(0, 4, int(rng.integers(gap // 2, gap))))
        parts.append(u)
    parts.append(rng.integers(0, 4, gap // 2))
    return LETTERS[np.concatenate(parts)].tobytes()


def replay(seed, same_genome, init_len):
    """Runs every window of a drawn pair of sequences in order.  After each window its surviving intervals go through the host
    forms of roll / filter / extend / filter, and the hits that pass are appended to `found` and added to the point-level tree,
    which is then trimmed as the reference trims it.  At every tree query both models are asked and must agree.  Returns what a
    call over the whole run takes and must answer: the arrays, the final list, the prefix of every window and of every interval,
    and the models' intervals and verdicts."""
    extz2 = ex()
    rng = np.random.default_rng(seed)
    unit = rng.integers(0, 4, int(rng.integers(180, 260)))
    qs = draw_sequence(rng, unit, 6, 1000)
    rs = qs if same_genome else draw_sequence(rng, unit, 7, 900)
    assert 3000 <= len(qs) <= 6000 and 3000 <= len(rs) <= 6000
    k, w = 8, 4
    q = S.records(M.get_minimizers(qs, k, w, True))
    r = q if same_genome else S.records(M.get_minimizers(rs, k, w, True))
    r_sorted = S.index_order(r)
    limit = [max(1, s // 8) for s in range(200)]
    kw = dict(r_threshold=BIG, len_q=len(qs), init_len=init_len, same_genome=same_genome, uppercase_seeds=1, limit=limit)
    pool, q_off, r_off = (qs, 0, 0) if same_genome else (qs + rs, 0, len(qs))
    # (max_sd_size keeps a hit near 2.5 windows: the point-level tree pays for every point of a times every point of b)
    fparams, eparams = extz2.filter_params(), extz2.extend_params(same_genome=bool(same_genome), max_sd_size=int(2.5 * init_len))
    min_read_size = init_len  # what initial_search passes
    walk = FM.Walker(q, r_sorted, **kw)
    tree, found = FM.PointTree(), []
    nq = len(q)
    visible, visible_iv, verdicts, all_T, all_rolls, windows, first = [], [], [], [], [], np.zeros(nq, S.WINDOW), [0]
    lost = 0
    for i in range(nq):
        visible.append(len(found))
        see = FM.RecordList(found, len(found))
        ans = walk.window(i, see.excluded)
        assert ans == walk.window(i, tree.excluded), i  # the two models, on the exclusions
        lost += len(ans[3]) < len(walk.window(i, lambda loc, pos: False)[3])
        qsz, nm, ng, c, flags, T = ans
        windows[i] = (qsz, nm, ng, len(c), flags)
        first.append(first[-1] + len(T))
        if T:
            T_arr = np.array(T, np.int64).astype("<i4").view(S.INTERVAL).reshape(-1)
            w1 = np.zeros(nq, S.WINDOW)
            w1[i] = windows[i]
            f1 = np.array([0] * (i + 1) + [len(T)] * (nq - i), np.uint64)
            code, rolls = extz2.search_roll_host(q, w1, f1, T_arr, r, len(rs), init_len, limit)
            assert code == 0
            code, tasks = extz2.search_filter_tasks_host(q, w1, f1, T_arr, rolls, len(qs), len(rs), init_len, q_off, 0, r_off, 0, 1)
            assert code == 0
            code, frec = extz2.search_filter_host(pool, tasks, fparams)
            assert code == 0
            code, hits = extz2.search_extend_host(q, w1, f1, T_arr, rolls, frec, r, len(qs), len(rs), init_len, limit, eparams)
            assert code == 0
            code, htasks = extz2.search_hit_tasks_host(hits, len(qs), len(rs), q_off, 0, r_off, 0)
            assert code == 0
            code, hrec = extz2.search_filter_host(pool, htasks, fparams)
            assert code == 0
            fail = extz2.FILTER_UPPER_FAIL | extz2.FILTER_QGRAM_FAIL | extz2.FILTER_SKIPPED
            pf_pos = int(q["loc"][i])
            for t in range(len(T)):
                visible_iv.append(len(found))
                args = (pf_pos, pf_pos + init_len, int(rolls["ref_start"][t]), int(rolls["ref_end"][t]), min_read_size)
                verdict = FM.RecordList(found, len(found)).is_overlap(*args)
                assert verdict == tree.is_overlap(*args), (i, t)  # the two models, on is_overlap
                verdicts.append(int(verdict))
                if rolls["jaccard"][t] < 0 or verdict or frec["flags"][t] & fail or hits["flags"][t] or hrec["flags"][t] & fail:
                    continue
                a = (int(hits["query_start"][t]), int(hits["query_end"][t]))
                b = (int(hits["ref_start"][t]), int(hits["ref_end"][t]))
                found.append(a + b)
                tree.add_hit(a, b)
            all_T.append(T_arr)
            all_rolls.append(rolls)
        tree.trim(int(q["loc"][i]) - min_read_size)
    cat = (lambda parts, dt: np.concatenate(parts) if parts else np.zeros(0, dt))
    return dict(q=q, r=r, r_sorted=r_sorted, kw=kw, found=FM.found_records(found), visible=np.array(visible, np.uint32),
                first=np.array(first, np.int64), windows=windows, intervals=cat(all_T, S.INTERVAL),
                rolls=cat(all_rolls, extz2.SEARCH_ROLL_DTYPE), visible_iv=np.array(visible_iv, np.uint32),
                verdicts=np.array(verdicts, np.uint32), min_read_size=min_read_size, lost=lost, len_r=len(rs), pool=pool,
                q_off=q_off, r_off=r_off)


REPLAYS = ((11, 0, 60), (13, 1, 90))  # (seed, same_genome, init_len); the seeds chosen so that the asserts below hold
_replays = {}


def replayed(which):
    if which not in _replays:
        _replays[which] = replay(*which)
    return _replays[which]


@pytest.mark.parametrize("which", REPLAYS)
def test_both_models_and_the_host_forms_agree_on_a_replay(which):
    R = replayed(which)
    # not vacuous: hits were added, a window lost a candidate to them, an interval was answered 1
    assert len(R["found"]) >= 5 and R["lost"] >= 1 and R["verdicts"].sum() >= 1, (len(R["found"]), R["lost"], R["verdicts"].sum())
    assert len(set(R["visible"].tolist())) >= 3 and 40 <= which[2] <= 100
    want = (R["first"], R["windows"], R["intervals"])
    same_records(host_windows(R["q"], R["r_sorted"], R["found"], R["visible"], **R["kw"]), want)
    same_records(FM.search_windows_found(R["q"], R["r_sorted"], found=R["found"], visible=R["visible"], **R["kw"]), want)
    got = host_overlap(R["q"], R["first"], R["rolls"], R["found"], R["visible_iv"], R["kw"]["init_len"], R["min_read_size"])
    assert np.array_equal(got, R["verdicts"])
    assert np.array_equal(FM.search_overlap(R["q"], R["first"], R["rolls"], R["found"], R["visible_iv"], R["kw"]["init_len"],
                                            R["min_read_size"]), R["verdicts"])


# ---- 3. hand-made edges, against the record-list model ----

def kwargs(**kw):
    base = dict(r_threshold=BIG, len_q=10 ** 9, init_len=100, same_genome=0, uppercase_seeds=1, limit=[1] * 64)
    base.update(kw)
    return base


def window_scenarios():
    """(name, q rows, r rows, found rows, visible, arguments, what the model's answer must show)."""
    out = []

    def add(name, q_rows, r_rows, found, visible, shows, **kw):
        out.append((name, S.records(q_rows), S.index_order(S.records(r_rows)), FM.found_records(found),
                    np.array(visible, np.uint32), kwargs(**kw), shows))

    def cands(a):
        return a[1]["n_candidates"].tolist()
    one_q, one_r = [(1, 50, 0)], [(1, 500, 0), (1, 900, 0)]
    # the member's loc at q_start is in, at q_end is out
    add("loc == q_start", one_q, one_r, [(50, 60, 400, 600)], [1], lambda a: cands(a) == [1])
    add("loc == q_end", one_q, one_r, [(40, 50, 400, 600)], [1], lambda a: cands(a) == [2])
    # pos at r_end - 1 is in, at r_end is out
    add("pos == r_end - 1", one_q, one_r, [(0, 100, 400, 501)], [1], lambda a: cands(a) == [1])
    add("pos == r_end", one_q, one_r, [(0, 100, 400, 500)], [1], lambda a: cands(a) == [2])
    add("pos == r_start", one_q, one_r, [(0, 100, 500, 501)], [1], lambda a: cands(a) == [1])
    # a record that reaches the window only at loc - qs == init_len: that member is inclusive
    far_q, far_r = [(1, 0, 0), (2, 100, 0), (3, 101, 0)], [(2, 500, 0), (3, 900, 0)]
    add("record at qs + init_len", far_q, far_r, [(100, 101, 0, 1000)], [1, 1, 1], lambda a: cands(a) == [0, 1, 1])
    add("record behind qs + init_len", far_q, far_r, [(101, 102, 0, 1000)], [1, 1, 1], lambda a: cands(a) == [1, 1, 0])
    # empty records on either axis are never visible
    add("empty on the query axis", one_q, one_r, [(50, 50, 0, 1000), (60, 40, 0, 1000)], [2], lambda a: cands(a) == [2])
    add("empty on the reference axis", one_q, one_r, [(0, 100, 500, 500), (0, 100, 900, 100)], [2], lambda a: cands(a) == [2])
    # one position gathered by two members: excluded for one, it survives; excluded for both, it does not
    two_q = [(1, 10, 0), (1, 30, 0)]
    add("excluded for one member of two", two_q, [(1, 500, 0)], [(0, 20, 400, 600)], [1, 1],
        lambda a: a[1]["n_gathered"].tolist() == [2, 1] and cands(a) == [1, 1])
    add("excluded for both members", two_q, [(1, 500, 0)], [(0, 20, 400, 600), (25, 35, 500, 501)], [2, 2], lambda a: cands(a) == [0, 0])
    # visible of 0, of nf, and cutting between two records that both match
    both = [(0, 100, 400, 600), (0, 100, 800, 1000)]
    add("visible 0", one_q, one_r, both, [0], lambda a: cands(a) == [2])
    add("visible cuts between two", one_q, one_r, both, [1], lambda a: cands(a) == [1])
    add("visible nf", one_q, one_r, both, [2], lambda a: cands(a) == [0] and a[0].tolist() == [0, 0])
    # the exclusion under same_genome, where the floor drops positions too
    add("with same_genome", [(1, 10, 0)], [(1, 100, 0), (1, 110, 0), (1, 300, 0)], [(0, 50, 290, 310)], [1],
        lambda a: a[1]["n_gathered"][0] == 3 and cands(a) == [1], same_genome=1)
    return out


def overlap_scenarios():
    """(name, q loc, (ref_start, ref_end), found rows, visible_iv, init_len, min_read_size, verdict)."""
    out = []

    def add(name, found, want, loc=1000, ref=(5000, 5100), vis=None, init_len=100, mrs=100):
        out.append((name, loc, ref, found, len(found) if vis is None else vis, init_len, mrs, want))
    add("total overlap", [(1000, 1100, 5000, 5100)], 1)
    add("total overlap misses by a base on the query", [(1000, 1099, 5000, 5100)], 0)
    add("total overlap misses by a base on the reference", [(1000, 1100, 5000, 5099)], 0)
    add("pf_pos at q_end", [(900, 1000, 5000, 5100)], 0)
    add("pfp_pos at r_end", [(1000, 1100, 4900, 5000)], 0)
    add("an empty record", [(1000, 1000, 5000, 5100), (1000, 1100, 5100, 5000)], 0)
    # the small-interval rule with an odd min_read_size: 701 * 1.5 = 1051.5 -- a smaller side of 1051 is skipped, 1052 goes on
    for small, want in ((1051, 0), (1052, 1)):
        add("smaller side %d" % small, [(900, 900 + small, 4000, 6000)], want, init_len=2000, mrs=701)
        add("smaller side %d on the reference" % small, [(0, 3000, 4950, 4950 + small)], want, init_len=2000, mrs=701, ref=(5000, 7000))
    # the allowance: eA - pf_pos at min_read_size and one below it, on either axis
    add("allowance met on both", [(500, 1300, 4000, 5300)], 1, init_len=400, mrs=300)
    add("allowance one short on the query", [(500, 1299, 4000, 5300)], 0, init_len=400, mrs=300)
    add("allowance one short on the reference", [(500, 1300, 4000, 5299)], 0, init_len=400, mrs=300)
    # total overlap answers 1 on a record that the small-interval rule would skip
    add("total overlap on a small record", [(1000, 1100, 5000, 5100)], 1, mrs=701)
    # a later record answers where an earlier one is skipped; the prefix decides
    pair = [(990, 1050, 4990, 5050), (1000, 1100, 5000, 5100)]
    add("the second record answers", pair, 1)
    add("the prefix ends before it", pair, 0, vis=1)
    add("nothing visible", pair, 0, vis=0)
    return out


def test_hand_made_window_edges():
    for name, q, r, found, visible, kw, shows in window_scenarios():
        want = FM.search_windows_found(q, r, found=found, visible=visible, **kw)
        assert shows(want), (name, want)
        same_records(host_windows(q, r, found, visible, **kw), want)


def overlap_arrays(cases):
    """One window with one interval per case, as the overlap call takes them."""
    extz2 = ex()
    q = S.records([(7, c[1], 0) for c in cases])
    first = np.arange(len(cases) + 1, dtype=np.uint64)
    rolls = np.zeros(len(cases), extz2.SEARCH_ROLL_DTYPE)
    rolls["ref_start"], rolls["ref_end"] = [c[2][0] for c in cases], [c[2][1] for c in cases]
    rolls["jaccard"], rolls["flags"] = -5, extz2.ROLL_WIDE  # (whatever its flags)
    return q, first, rolls


def test_hand_made_overlap_edges():
    for name, loc, ref, found, vis, init_len, mrs, want in overlap_scenarios():
        q, first, rolls = overlap_arrays([(name, loc, ref)])
        found = FM.found_records(found)
        model = FM.search_overlap(q, first, rolls, found, [vis], init_len, mrs)
        assert model.tolist() == [want], name
        assert host_overlap(q, first, rolls, found, [vis], init_len, mrs).tolist() == [want], name


def test_a_verdict_that_depends_on_the_intervals_own_prefix():
    """Two intervals of ONE window, the same rolled place: the first sees no record, the second sees the hit the first made."""
    extz2 = ex()
    q = S.records([(7, 1000, 0), (8, 2000, 0)])
    first = np.array([0, 2, 3], np.uint64)
    rolls = np.zeros(3, extz2.SEARCH_ROLL_DTYPE)
    rolls["ref_start"], rolls["ref_end"] = [5000, 5020, 5000], [5100, 5120, 5100]
    found = FM.found_records([(900, 1200, 4900, 5200)])
    for vis, want in (([0, 1, 1], [0, 1, 0]), ([1, 0, 0], [1, 0, 0]), ([1, 1, 1], [1, 1, 0])):
        assert FM.search_overlap(q, first, rolls, found, vis, 100, 100).tolist() == want
        assert host_overlap(q, first, rolls, found, vis, 100, 100).tolist() == want


def wide_found(n, qs=5000, init_len=100):
    """n records that meet the window at qs (spread over its span, the last at qs + init_len exactly), two that do not, and an
    empty one; the first record covers the position 700 for the member at qs."""
    rows = [(qs, qs + 1, 690, 710)]
    rows += [(qs - 50 + (t % (init_len + 50)), qs + 1 + (t % (init_len + 50)), 10 ** 6, 10 ** 6 + 5) for t in range(n - 2)]
    rows += [(qs + init_len, qs + init_len + 9, 10 ** 6, 10 ** 6 + 5)]
    rows += [(qs + init_len + 1, qs + init_len + 9, 0, 10 ** 7), (qs - 9, qs, 0, 10 ** 7), (qs, qs + 50, 800, 800)]
    assert n >= 3
    return FM.found_records(rows)


def wide_case(n):
    q = S.records([(1, 5000, 0), (2, 5050, 0), (1, 9000, 0)])
    r = S.index_order(S.records([(1, 700, 0), (1, 720, 0), (2, 705, 0)]))
    found = wide_found(n)
    return q, r, found, np.array([len(found), len(found), len(found)], np.uint32), kwargs()


def test_found_wide_is_flagged_and_completed_by_the_host_form():
    for n in (256, 257):
        q, r, found, visible, kw = wide_case(n)
        want = FM.search_windows_found(q, r, found=found, visible=visible, **kw)
        assert bool(want[1]["flags"][0] & FM.FOUND_WIDE) == (n > 256) and want[1]["flags"][2] == 0
        assert want[1]["n_gathered"].tolist() == [3, 1, 2] and want[1]["n_candidates"].tolist() == [2, 1, 2]  # (700 is dropped for window 0)
        same_records(host_windows(q, r, found, visible, **kw), want)


# ---- 4. refusals ----

def test_refusals():
    extz2 = ex()
    lib = extz2.load_library()
    q, r = S.records([(1, 50, 0), (2, 60, 0)]), S.index_order(S.records([(1, 500, 0)]))
    found = FM.found_records([(0, 100, 4000, 6000)])
    vis = np.array([1, 1], np.uint32)
    kw = kwargs()

    def wcode(found=found, visible=vis, **change):
        return extz2.search_windows_found_host(q, r, found=found, visible=visible, **dict(kw, **change))[0]
    assert wcode() == 0
    assert wcode(init_len=0) == SDF_ERR_INVALID and wcode(init_len=(1 << 30) + 1) == SDF_ERR_UNSUPPORTED
    assert wcode(limit=[0, 3, 0]) == SDF_ERR_UNSUPPORTED
    assert wcode(visible=np.array([1, 2], np.uint32)) == SDF_ERR_INVALID  # a prefix longer than the list
    limit = np.array(kw["limit"], np.int32)
    first, windows, used = np.zeros(3, np.uint64), np.zeros(2, S.WINDOW), C.c_size_t(0)
    good = [q.ctypes.data, 2, 10 ** 9, r.ctypes.data, 1, BIG, 100, 0, 1, limit.ctypes.data, len(limit), found.ctypes.data, 1,
            vis.ctypes.data, first.ctypes.data, windows.ctypes.data, None, 0, C.byref(used)]
    assert lib.sdf_search_windows_found_host(*good) == SDF_ERR_OVERFLOW and used.value == 1
    for at in (0, 3, 9, 11, 13, 14, 15, 18):
        bad = list(good)
        bad[at] = None
        assert lib.sdf_search_windows_found_host(*bad) == SDF_ERR_INVALID, at
    bad = list(good)
    bad[12] = 1 << 31  # nf > 2^31 - 1: refused before the list is read
    assert lib.sdf_search_windows_found_host(*bad) == SDF_ERR_UNSUPPORTED
    bad = list(good)
    bad[11], bad[12] = None, 0  # no record and no list: fine
    zero = np.zeros(2, np.uint32)
    bad[13] = zero.ctypes.data
    assert lib.sdf_search_windows_found_host(*bad) == SDF_ERR_OVERFLOW
    # more than 2^31 - 1 bin entries: 4,097 records over the whole query axis, 2^19 bins each
    many = FM.found_records([(0, 2 ** 31 - 1, 0, 10)] * 4097)
    assert extz2.found_entries(many) == 4097 << 19 and extz2.found_entries(many[:4095]) < 2 ** 31
    assert wcode(found=many, visible=np.array([0, 0], np.uint32)) == SDF_ERR_UNSUPPORTED
    assert extz2.found_entries(FM.found_records([(4095, 4097, 0, 1), (4096, 4096, 0, 1), (0, 4096, 0, 1), (0, 9, 5, 5)])) == 3

    # the overlap call
    first = np.array([0, 1, 2], np.uint64)
    rolls = np.zeros(2, extz2.SEARCH_ROLL_DTYPE)
    out = np.zeros(2, np.uint32)

    def ocode(*args):
        return lib.sdf_search_overlap_host(*args)
    good = [q.ctypes.data, 2, first.ctypes.data, rolls.ctypes.data, found.ctypes.data, 1, vis.ctypes.data, 100, 100, out.ctypes.data]
    assert ocode(*good) == 0
    for at in (0, 2, 3, 4, 6, 9):
        bad = list(good)
        bad[at] = None
        assert ocode(*bad) == SDF_ERR_INVALID, at
    for at, value, want in ((7, 0, SDF_ERR_INVALID), (7, (1 << 30) + 1, SDF_ERR_UNSUPPORTED), (8, -1, SDF_ERR_INVALID),
                            (5, 1 << 31, SDF_ERR_UNSUPPORTED)):
        bad = list(good)
        bad[at] = value
        assert ocode(*bad) == want, (at, value)
    assert ocode(*(good[:8] + [0] + good[9:])) == 0  # min_read_size 0 is allowed
    over = np.array([1, 2], np.uint32)
    assert ocode(*(good[:6] + [over.ctypes.data] + good[7:])) == SDF_ERR_INVALID
    for bad_first in ([1, 1, 2], [0, 2, 1]):
        bf = np.array(bad_first, np.uint64)
        assert ocode(*(good[:2] + [bf.ctypes.data] + good[3:])) == SDF_ERR_INVALID
    huge = np.array([0, 0, 1 << 31], np.uint64)
    assert ocode(*(good[:2] + [huge.ctypes.data] + good[3:])) == SDF_ERR_UNSUPPORTED
    assert ocode(*(good[:4] + [many.ctypes.data, len(many)] + good[6:])) == SDF_ERR_UNSUPPORTED
    assert ocode(None, 0, None, None, None, 0, None, 100, 100, None) == 0  # nq == 0


def test_library_exports_the_entry_points_and_record_sizes():
    extz2 = ex()
    lib = extz2.load_library()
    for name in ("sdf_search_windows_found", "sdf_search_windows_found_device", "sdf_search_windows_found_host", "sdf_search_overlap",
                 "sdf_search_overlap_device", "sdf_search_overlap_host", "sdf_search_found_entries"):
        assert hasattr(lib, name), name
    assert extz2.SEARCH_FOUND_DTYPE == FM.FOUND and (extz2.SEARCH_FOUND_WIDE, extz2.SEARCH_MAX_FOUND) == (FM.FOUND_WIDE, FM.MAX_FOUND)
