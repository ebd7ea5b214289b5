"""The search extension on the device: every rolled interval grown to its hit (sdf_search_extend, sdf_search_extend_device,
sdf_search_hit_tasks_device; sedef_amd/csrc/search_extend.hip).

Expected values: the reference's own answers (tests/golden/search_extend_kat.json.gz), sdf_search_extend_host and
tests/extend_model.py, which tests/test_search_extend_cpu.py checks against that fixture.  Every comparison is exact."""
import os
import sys

import numpy as np
import pytest
import torch  # (at collection: before the library brings a HIP runtime of its own along)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import extend_model as E  # noqa: E402
import minim_model as M  # noqa: E402
import roll_model as R  # noqa: E402
import search_model as S  # noqa: E402
from test_search_extend_cpu import (case_expected, case_extend_inputs, case_params, host, load_fixture, random_extend_inputs,  # noqa: E402
                                    same_hits, wide_growth_inputs)
from test_search_windows_cpu import case_args  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 4  # records of 0xEE behind d_out[n_max]


@pytest.fixture(scope="module")
def eng():
    import sedef_amd
    e = sedef_amd.Extz2Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def kat():
    return load_fixture()


def up(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy() if len(a) else np.zeros(8, np.uint8)).cuda()


def device_form(eng, args, params, n_max=None):
    """sdf_search_extend_device on arrays uploaded here: (the records below n_max, the bytes behind them)."""
    from sedef_amd import extz2
    q, windows, first, intervals, rolls, filt, r, len_q, len_r, init_len, limit = args
    n_max = int(first[-1]) if n_max is None else n_max
    d = [up(q), up(windows), up(np.asarray(first, np.uint64)), up(intervals), up(np.ascontiguousarray(rolls, extz2.SEARCH_ROLL_DTYPE)),
         up(r), up(np.asarray(limit, np.int32))]
    d_filt = None if filt is None else up(np.ascontiguousarray(filt, extz2.FILTER_REC_DTYPE))
    d_out = torch.full(((n_max + GUARD) * 40,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # (the tensors were filled on torch's stream)
    eng.search_extend_device(d[0].data_ptr(), len(q), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(),
                             None if d_filt is None else d_filt.data_ptr(), n_max, d[5].data_ptr(), len(r), len_q, len_r, init_len,
                             d[6].data_ptr(), len(limit), d_out.data_ptr(), extz2.extend_params(**params))
    raw = d_out.cpu().numpy().tobytes()
    return np.frombuffer(raw[:40 * n_max], E.HIT), raw[40 * n_max:]


def as_device(want):
    expect = want.copy()
    wide = (want["flags"] & E.WIDE) != 0
    expect[wide] = (0,) * 9 + (E.WIDE,)
    return expect


def check_both(eng, args, params, want=None):
    """The device form and the combined form against `want` (default: the host form); a WIDE interval is empty from the device."""
    from sedef_amd import extz2
    if want is None:
        code, want = host(args, params)
        assert code == 0
    dev, behind = device_form(eng, args, params)
    same_hits(dev, as_device(want), "device form")
    assert behind == b"\xEE" * (40 * GUARD)
    code, got = eng.search_extend_raw(*args, extz2.extend_params(**params))
    assert code == 0, eng.lib.sdf_last_error(eng.ctx).decode()
    same_hits(got, want, "combined form")
    return want


def test_fixture_record_for_record(eng, kat):
    n = 0
    for c in kat["cases"]:
        args, params = case_extend_inputs(c)
        n += int((check_both(eng, args, params, case_expected(c))["flags"] == 0).sum())
    assert n >= 2000


def test_random_small_alphabet_inputs_against_the_host_form(eng):
    rng = np.random.default_rng(22)
    n = 0
    for it in range(10):
        args = random_extend_inputs(rng, nq=int(rng.choice([1, 40, 90])), nr=int(rng.choice([5, 160, 380])), hashes=int(rng.choice([3, 9, 40])),
                                    init_len=int(rng.choice([1, 6, 25, 90])), dup_locs=bool(it % 3 == 2))
        if it % 3 == 1:
            args = args[:5] + (None,) + args[6:]  # a null filter array
        params = dict(max_error=float(rng.choice([0.3, 0.25])), max_edit_error=float(rng.choice([0.15, 0.05])),
                      max_sd_size=int(rng.choice([1 << 20, 300])), same_genome=it % 2 == 0)
        n += len(check_both(eng, args, params))
    assert n > 300


def test_a_null_filter_array_and_one_that_stops_intervals(eng, kat):
    c = next(c for c in kat["cases"] if c["name"] == "k12 1")
    args, params = case_extend_inputs(c)
    from sedef_amd import extz2
    filt = np.zeros(len(args[4]), extz2.FILTER_REC_DTYPE)
    filt["flags"] = np.resize([0, 1, 4, 2, 0, 8, 0], len(filt))
    stopped = check_both(eng, args[:5] + (filt,) + args[6:], params)
    plain = case_expected(c)
    stops = (filt["flags"] & E.FILTER_STOPS) != 0
    assert (stopped["flags"][stops] == E.SKIPPED).all() and stopped[~stops].tobytes() == plain[~stops].tobytes()
    assert (plain["flags"][stops] == 0).sum() > 10


def test_chained_on_one_stream_to_the_second_filter(eng, kat):
    """windows -> roll -> filter tasks -> filter -> extend -> hit tasks -> filter on the caller's stream, one synchronisation
    at the end; every array stays on the device in between."""
    from sedef_amd import extz2
    c = next(c for c in kat["cases"] if c["name"] == "k12 0")
    args, params = case_extend_inputs(c)
    q, windows, first, intervals, rolls, _, r, len_q, len_r, init_len, limit = args
    kw = case_args(c)
    q_text, r_text = c["q"].encode(), c["r"].encode()
    pool = b"gattaca" + q_text + b"NNNcat" + r_text + b"acgt"
    q_off, r_off = 7, 7 + len(q_text) + 6
    eng.pool_upload(pool)
    eng.lib.sdf_pool_sync(eng.ctx)
    n, cap = len(intervals), len(intervals) + 50
    d_q, d_rs, d_r, d_limit = up(q), up(S.index_order(r)), up(r), up(limit)
    d_first = torch.zeros(len(q) + 1, dtype=torch.int64, device="cuda")

    def room(size, fill=0):
        return torch.full((cap * size + 64,), fill, dtype=torch.uint8, device="cuda")
    d_win = torch.zeros(len(q) * 20, dtype=torch.uint8, device="cuda")
    d_iv, d_rolls, d_tasks, d_recs, d_hits, d_tasks2, d_recs2 = room(8), room(24), room(32), room(20), room(40, 0xEE), room(32), room(20)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    st = stream.cuda_stream
    fp = extz2.filter_params()
    eng.search_windows_device(d_q.data_ptr(), len(q), len_q, d_rs.data_ptr(), len(r), kw["r_threshold"], init_len, kw["same_genome"],
                              kw["uppercase_seeds"], d_limit.data_ptr(), len(limit), d_first.data_ptr(), d_win.data_ptr(), d_iv.data_ptr(),
                              cap, stream=st)
    eng.search_roll_device(d_q.data_ptr(), len(q), d_win.data_ptr(), d_first.data_ptr(), d_iv.data_ptr(), cap, d_r.data_ptr(), len(r), len_r,
                           init_len, d_limit.data_ptr(), len(limit), d_rolls.data_ptr(), stream=st)
    eng.search_filter_tasks_device(d_q.data_ptr(), len(q), d_win.data_ptr(), d_first.data_ptr(), d_iv.data_ptr(), d_rolls.data_ptr(), cap,
                                   len_q, len_r, init_len, q_off, False, r_off, False, True, d_tasks.data_ptr(), stream=st)
    eng.search_filter_device(d_tasks.data_ptr(), cap, False, d_recs.data_ptr(), fp, stream=st)
    eng.search_extend_device(d_q.data_ptr(), len(q), d_win.data_ptr(), d_first.data_ptr(), d_iv.data_ptr(), d_rolls.data_ptr(),
                             d_recs.data_ptr(), cap, d_r.data_ptr(), len(r), len_q, len_r, init_len, d_limit.data_ptr(), len(limit),
                             d_hits.data_ptr(), extz2.extend_params(**params), stream=st)
    eng.search_hit_tasks_device(d_hits.data_ptr(), cap, d_first.data_ptr() + 8 * len(q), len_q, len_r, q_off, False, r_off, False,
                                d_tasks2.data_ptr(), stream=st)
    eng.search_filter_device(d_tasks2.data_ptr(), cap, False, d_recs2.data_ptr(), fp, stream=st)
    stream.synchronize()
    assert int(d_first.cpu()[-1]) == n and n > 100

    def down(t, dtype):
        return np.frombuffer(t.cpu().numpy().tobytes()[:cap * dtype.itemsize], dtype)
    # the same on the host: the fixture's rolls, the filter's host form over the same pool
    code, tasks = extz2.search_filter_tasks_host(q, windows, first, intervals, rolls, len_q, len_r, init_len, q_off, False, r_off, False, True)
    assert code == 0
    code, recs = extz2.search_filter_host(pool, tasks)
    assert code == 0
    assert down(d_recs, extz2.FILTER_REC_DTYPE)[:n].tobytes() == recs.tobytes()
    code, hits = host(args[:5] + (recs,) + args[6:], params)
    assert code == 0 and (hits["flags"] == 0).sum() > 50
    raw = d_hits.cpu().numpy().tobytes()
    same_hits(np.frombuffer(raw[:40 * n], E.HIT), as_device(hits))
    assert raw[40 * n:] == b"\xEE" * (len(raw) - 40 * n)  # the wavefronts beyond first[nq] wrote nothing
    code, tasks2 = extz2.search_hit_tasks_host(as_device(hits), len_q, len_r, q_off, False, r_off, False)
    assert code == 0
    got_tasks = down(d_tasks2, extz2.FILTER_TASK_DTYPE)
    assert got_tasks[:n].tobytes() == tasks2.tobytes() and (got_tasks["flags"][n:] == 4).all()
    code, recs2 = extz2.search_filter_host(pool, tasks2)
    assert code == 0
    got_recs = down(d_recs2, extz2.FILTER_REC_DTYPE)
    assert got_recs[:n].tobytes() == recs2.tobytes() and (got_recs["flags"][n:] == 8).all()
    assert ((recs2["flags"] & 8) == 0).sum() > 50


def test_engine_search_extend_on_an_uploaded_pool(eng, kat):
    """Extz2Engine.search_extend chains minimizers, index, windows, roll, filter, extend, hit tasks and the second filter on two
    ranges of the resident pool; a reversed reference lies there as the fixture has it.  Against the host forms, step by step."""
    from sedef_amd import extz2
    picked = [c for c in kat["cases"] if c["k"] == 12] + kat["cases"][:6]
    assert any(c["same"] for c in picked) and any(c["r_rc"] for c in picked)
    n_hits = n_passed = 0
    for c in picked:
        args, params = case_extend_inputs(c)
        q, windows, first, intervals, rolls, _, r, len_q, len_r, init_len, limit = args
        q_text = c["q"].encode()
        pool = b"gattaca" + q_text + b"NNNcat"
        q_range = r_range = (7, len(q_text))
        if not c["same"]:
            r_range = (len(pool), len(c["r"]), bool(c["r_rc"]))
            pool += c["r"].encode() + b"acgt"
        eng.pool_upload(pool)
        got = eng.search_extend(q_range, r_range, c["k"], c["w"], c["sl"], init_len, c["same_genome"], c["uppercase_seeds"], c["limit"],
                                r_threshold=c["threshold"], extend=extz2.extend_params(**params))
        g_first, g_windows, g_intervals, g_rolls, g_recs, g_hits, g_hit_recs = got
        assert np.array_equal(g_first, first) and g_intervals.tobytes() == np.ascontiguousarray(intervals, extz2.SEARCH_INTERVAL_DTYPE).tobytes()
        assert g_rolls.tobytes() == np.ascontiguousarray(rolls, extz2.SEARCH_ROLL_DTYPE).tobytes(), c["name"]
        strands = (int(q_range[0]), False, int(r_range[0]), len(r_range) > 2 and r_range[2])
        code, tasks = extz2.search_filter_tasks_host(q, windows, first, intervals, rolls, len_q, len_r, init_len, *strands, True)
        assert code == 0
        code, recs = extz2.search_filter_host(pool, tasks)
        assert code == 0 and g_recs.tobytes() == recs.tobytes(), c["name"]
        code, hits = host(args[:5] + (recs,) + args[6:], params)
        assert code == 0
        same_hits(g_hits, hits, c["name"])
        code, tasks2 = extz2.search_hit_tasks_host(hits, len_q, len_r, *strands)
        assert code == 0
        code, recs2 = extz2.search_filter_host(pool, tasks2)
        assert code == 0 and g_hit_recs.tobytes() == recs2.tobytes(), c["name"]
        n_hits += int((hits["flags"] == 0).sum())
        n_passed += int((recs2["flags"] & (1 | 2 | 8) == 0).sum())
    assert n_hits > 100 and n_passed > 20


def grown(args, hits, t):
    """By how many records the four ends of interval t's winnow ranges moved beyond their entry values."""
    q, windows, first, intervals, rolls = args[:5]
    i = int(np.searchsorted(first, t, "right")) - 1
    h = hits[t]
    return (i - h["q_winnow_start"], h["q_winnow_end"] - (i + windows["n_members"][i]), rolls["winnow_start"][t] - h["r_winnow_start"],
            h["r_winnow_end"] - rolls["winnow_end"][t])


def identical_sequences(records, count, i, init_len=12):
    """Two identical sequences at k = 3, w = 2 -- a record every base or two --, cut behind `count` records, and the one
    interval of window i."""
    q = records[:count].copy()
    n_bases = int(q["loc"][-1]) + 3
    nm = int(np.searchsorted(q["loc"], q["loc"][i] + init_len, "right")) - i
    windows = np.zeros(len(q), S.WINDOW)
    windows["n_members"], windows["query_size"] = 1, 1
    windows[i] = (len(set(R.keys_of(q[i:i + nm]))), nm, 0, 0, 0)
    first = np.zeros(len(q) + 1, np.int64)
    first[i + 1:] = 1
    intervals = np.array([(q["loc"][i], q["loc"][i] + 1)], S.INTERVAL)
    limit = np.maximum(1, np.arange(400) // 4).astype(np.int32)
    rolls = R.search_roll(q, windows, first, intervals, q, n_bases, init_len, limit)
    return q, windows, first, intervals, rolls, None, q, n_bases, n_bases, init_len, limit


def test_growth_cap_at_its_value_and_one_more(eng):
    """The extension of two identical random sequences runs to both sequence ends; they are cut so that the widest growth of a
    winnow range is exactly SDF_EXTEND_MAX_GROW -- answered by the kernel --, then one more -- flagged by the device form and
    completed, equal to the host form, by sdf_search_extend.

    The sequences are cut by RECORDS, not by bases: the arrays are the first `count` minimizers of one random k = 3, w = 2
    sequence and the length is set to the last loc + 3, so they are not exactly the minimizers of a sequence of that length
    (the last window of a real one could differ).  That moves the growth by exactly one record from one case to the next,
    which a length in bases cannot promise; the cap is exercised the same."""
    from sedef_amd import extz2
    cap = extz2.EXTEND_MAX_GROW
    seq = bytes(np.random.default_rng(5).choice(np.frombuffer(b"ACGT", np.uint8), 6 * cap + 800))
    records = S.records(M.get_minimizers(seq, 3, 2, True))
    i = cap - 2
    members_end = int(np.searchsorted(records["loc"], records["loc"][i] + 12, "right"))
    assert len(records) > members_end + cap + 1
    for over in (0, 1):
        args = identical_sequences(records, members_end + cap + over, i)
        code, hits = host(args, {})
        assert code == 0 and hits["q_winnow_start"][0] == 0 and hits["q_winnow_end"][0] == len(args[0]), "the extension reaches both ends"
        assert int(max(grown(args, hits, 0))) == cap + over and int(hits["flags"][0]) == (E.WIDE if over else 0)
        dev, _ = device_form(eng, args, {})
        same_hits(dev, as_device(hits), "growth == cap + %d, device form" % over)
        code, got = eng.search_extend_raw(*args)
        assert code == 0
        same_hits(got, hits, "growth == cap + %d, combined form" % over)


def test_growth_first_then_the_end_of_the_limit_table(eng):
    """The device form ends at the growth cap and says WIDE; sdf_search_extend completes the interval on the host, where a later
    add needs the table beyond its end: WIDE | NOLIMIT, the flag kept.  A table that ends first: NOLIMIT alone, from both."""
    args, n = wide_growth_inputs()
    for n_limit, flags in ((2 * E.MAX_GROW + 12, E.WIDE | E.NOLIMIT), (200, E.NOLIMIT)):
        short = args[:-1] + (args[-1][:n_limit],)
        want = check_both(eng, short, {})
        assert want[0].tolist() == (0,) * 9 + (flags,)


def test_n_max_above_and_below_the_interval_count(eng):
    rng = np.random.default_rng(23)
    args = random_extend_inputs(rng, nq=90, nr=380)
    n = int(args[2][-1])
    code, want = host(args, {})
    assert code == 0 and n > 20
    for n_max in (n + 7, n - 5, 1):
        dev, behind = device_form(eng, args, {}, n_max=n_max)
        m = min(n, n_max)
        same_hits(dev[:m], as_device(want)[:m], n_max)
        assert dev[m:].tobytes() == b"\xEE" * (40 * (n_max - m)) and behind == b"\xEE" * (40 * GUARD)


def test_empty_inputs_launch_nothing(eng):
    from sedef_amd import extz2
    rng = np.random.default_rng(24)
    args = random_extend_inputs(rng)
    code, _ = eng.search_extend_raw(*args)
    assert code == 0
    before = eng.last_launches()
    none = np.zeros(len(args[0]) + 1, np.int64)
    code, got = eng.search_extend_raw(args[0], args[1], none, args[3][:0], args[4][:0], None, *args[6:])
    assert code == 0 and len(got) == 0
    code, got = eng.search_extend_raw(args[0][:0], args[1][:0], none[:1], args[3][:0], args[4][:0], None, *args[6:])
    assert code == 0
    eng.search_extend_device(1, len(args[0]), 1, 1, 1, 1, None, 0, 1, 5, 100, 100, 10, 1, 5, 1)
    eng.search_hit_tasks_device(1, 0, None, 100, 100, 0, False, 0, False, 1)
    assert eng.last_launches() == before
    # a refusal launches nothing either
    code, _ = eng.search_extend_raw(*args, extz2.extend_params(max_error=0.1))
    assert code == -4 and eng.last_launches() == before


def test_windows_at_the_first_and_the_last_minimizer(eng):
    """qws == 0 and qwe == nq at the entry: the left and the right prechecks fail from the first round on."""
    rng = np.random.default_rng(25)
    n = 0
    for it in range(4):
        q, windows, first, intervals, rolls, filt, r, len_q, len_r, init_len, limit = random_extend_inputs(rng, nq=40, nr=200)
        nq = len(q)
        windows["n_members"][nq - 1] = 1
        windows["n_members"][nq - 3] = 3
        rows, first = [], [0]
        for i in range(nq):
            if i in (0, nq - 3, nq - 1):
                rows += [(int(s), int(s) + 30) for s in rng.integers(0, len_r - 40, 3)]
            first.append(len(rows))
        intervals = np.array(rows, S.INTERVAL)
        first = np.array(first, np.int64)
        rolls = R.search_roll(q, windows, first, intervals, r, len_r, init_len, limit)
        want = check_both(eng, (q, windows, first, intervals, rolls, None, r, len_q, len_r, init_len, limit), {})
        live = want["flags"] == 0
        n += int((want["q_winnow_start"][live] == 0).sum()) + int((want["q_winnow_end"][live] == nq).sum())
    assert n > 6
