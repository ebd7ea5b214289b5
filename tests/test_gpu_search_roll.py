"""The search roll on the device: every reference interval rolled to its best initial match (sdf_search_roll,
sdf_search_roll_device; sedef_amd/csrc/search_roll.hip).

Expected values: the reference's own answers (tests/golden/search_roll_kat.json.gz), sdf_search_roll_host and
tests/roll_model.py, which tests/test_search_roll_cpu.py checks against that fixture.  Every comparison is exact."""
import os
import sys

import numpy as np
import pytest
import torch  # (at collection: before the library brings a HIP runtime of its own along)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import minim_model as M  # noqa: E402
import roll_model as R  # noqa: E402
import search_model as S  # noqa: E402
from test_search_roll_cpu import case_expected, case_inputs, host, load_fixture, random_inputs, same_rolls  # noqa: E402
from test_search_windows_cpu import case_args  # noqa: E402

pytestmark = pytest.mark.gpu

SDF_ERR_INVALID = -4
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


def device_form(eng, q, windows, first, intervals, r, len_r, init_len, limit, n_max=None, stream=None):
    """sdf_search_roll_device on arrays uploaded here: (the records below n_max, the bytes behind them)."""
    n_max = int(first[-1]) if n_max is None else n_max
    d = [up(q), up(windows), up(np.asarray(first, np.uint64)), up(intervals), up(r), up(np.asarray(limit, np.int32))]
    d_out = torch.full(((n_max + GUARD) * 24,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # (the tensors were filled on torch's stream)
    eng.search_roll_device(d[0].data_ptr(), len(q), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), n_max, d[4].data_ptr(), len(r),
                           len_r, init_len, d[5].data_ptr(), len(limit), d_out.data_ptr(), stream.cuda_stream if stream is not None else None)
    if stream is not None:
        stream.synchronize()
    raw = d_out.cpu().numpy().tobytes()
    return np.frombuffer(raw[:24 * n_max], R.ROLL), raw[24 * n_max:]


def check_both(eng, args, want=None):
    """The device form and the combined form against `want` (default: the host form); a WIDE interval is empty from the device."""
    if want is None:
        code, want = host(*args)
        assert code == 0
    dev, behind = device_form(eng, *args)
    expect = want.copy()
    wide = (want["flags"] & R.WIDE) != 0
    expect[wide] = (0, 0, 0, 0, 0, R.WIDE)
    same_rolls(dev, expect, "device form")
    assert behind == b"\xEE" * (24 * GUARD)
    code, got = eng.search_roll_raw(*args)
    assert code == 0, eng.lib.sdf_last_error(eng.ctx).decode()
    same_rolls(got, want, "combined form")
    return want


def test_fixture_record_for_record(eng, kat):
    n = 0
    for c in kat["cases"]:
        want = check_both(eng, case_inputs(c), case_expected(c))
        n += len(want)
    assert n >= 2000


def test_fixture_through_an_uploaded_pool(eng, kat):
    """search_roll chains minimizers, index, search_windows and the roll on ranges of the resident pool; a reversed reference
    lies there as the fixture has it."""
    picked = [c for c in kat["cases"] if c["k"] == 12] + kat["cases"][:8]
    assert any(c["same"] for c in picked) and any(c["r_rc"] for c in picked)
    for c in picked:
        q_text = c["q"].encode()
        pool = b"gattaca" + q_text + b"NNNcat"
        q_range = r_range = (7, len(q_text))
        if not c["same"]:
            r_range = (len(pool), len(c["r"]), bool(c["r_rc"]))
            pool += c["r"].encode() + b"acgt"
        eng.pool_upload(pool)
        first, windows, intervals, rolls = eng.search_roll(q_range, r_range, c["k"], c["w"], c["sl"], c["init_len"], c["same_genome"],
                                                           c["uppercase_seeds"], c["limit"], r_threshold=c["threshold"])
        assert [list(t) for t in zip(intervals["start"].tolist(), intervals["end"].tolist())] == [t[:2] for w in c["windows"] for t in w[2]]
        same_rolls(rolls, case_expected(c), c["name"])


def test_random_small_alphabet_inputs_against_the_host_form(eng):
    rng = np.random.default_rng(21)
    for it in range(12):
        args = random_inputs(rng, nq=int(rng.choice([1, 40, 90])), nr=int(rng.choice([5, 160, 380])), hashes=int(rng.choice([3, 9, 40])),
                             init_len=int(rng.choice([1, 6, 25, 90])), dup_locs=bool(it % 3 == 2))
        check_both(eng, args)


def test_chained_behind_search_windows_device_on_one_stream(eng, kat):
    """Both device calls on the caller's stream, no host read in between: the roll takes d_first, d_windows and the intervals as
    sdf_search_windows_device leaves them."""
    c = next(c for c in kat["cases"] if c["name"] == "k12 0")
    q, windows, first, intervals, r, len_r, init_len, limit = case_inputs(c)
    kw = case_args(c)
    cap = len(intervals) + 50  # (n_max: what the caller has room for)
    d_q, d_rs, d_r, d_limit = up(q), up(S.index_order(r)), up(r), up(limit)
    d_first = torch.zeros(len(q) + 1, dtype=torch.int64, device="cuda")
    d_win = torch.zeros(len(q) * 20, dtype=torch.uint8, device="cuda")
    d_iv = torch.zeros(cap * 8, dtype=torch.uint8, device="cuda")
    d_out = torch.full(((cap + GUARD) * 24,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    eng.search_windows_device(d_q.data_ptr(), len(q), kw["len_q"], d_rs.data_ptr(), len(r), kw["r_threshold"], init_len, kw["same_genome"],
                              kw["uppercase_seeds"], d_limit.data_ptr(), len(limit), d_first.data_ptr(), d_win.data_ptr(), d_iv.data_ptr(),
                              cap, stream=stream.cuda_stream)
    eng.search_roll_device(d_q.data_ptr(), len(q), d_win.data_ptr(), d_first.data_ptr(), d_iv.data_ptr(), cap, d_r.data_ptr(), len(r), len_r,
                           init_len, d_limit.data_ptr(), len(limit), d_out.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    raw = d_out.cpu().numpy().tobytes()
    n = len(intervals)
    assert n > 100 and int(d_first.cpu()[-1]) == n
    same_rolls(np.frombuffer(raw[:24 * n], R.ROLL), case_expected(c))
    assert raw[24 * n:] == b"\xEE" * (24 * (cap - n + GUARD))  # the wavefronts beyond first[nq] wrote nothing


def test_n_max_above_and_below_the_interval_count(eng):
    args = random_inputs(np.random.default_rng(5), nq=80)
    code, want = host(*args)
    n = len(want)
    assert code == 0 and n > 40
    for n_max in (n + 70, n, n - 1, n // 2, 1):
        got, behind = device_form(eng, *args, n_max=n_max)
        same_rolls(got[:min(n, n_max)], want[:min(n, n_max)], n_max)
        assert got[n:].tobytes() == b"\xEE" * (24 * max(0, n_max - n)) and behind == b"\xEE" * (24 * GUARD), n_max


def dense_reference(rng, n, k=10):
    """w = 1: a minimizer at about every second base."""
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()
    r = S.records(M.get_minimizers(seq, k, 1, True))
    assert 5 * len(r) >= 2 * n
    return seq, r


def test_span_cap_at_3072_and_one_more(eng):
    rng = np.random.default_rng(8)
    seq, r = dense_reference(rng, 9000)
    q = S.records(M.get_minimizers(seq[2000:2600], 10, 1, True))  # (the query is a piece of the reference: keys meet)
    init_len = 300
    windows = np.zeros(len(q), S.WINDOW)
    windows["n_members"], windows["query_size"] = 1, 1
    nm = 250
    windows[0] = (len(set(R.keys_of(q[:nm]))), nm, 0, 0, 0)
    first = np.zeros(len(q) + 1, np.int64)
    first[1:] = 2
    # one long merged interval: the last record with loc <= end + init_len is the 3,072nd from start on, and the one behind it
    locs = r["loc"].tolist()
    at = int(np.searchsorted(r["loc"], 1000))
    intervals = np.array([(1000, locs[at + 3071] - init_len), (1000, locs[at + 3072] - init_len)], S.INTERVAL)
    args = (q, windows, first, intervals, r, len(seq), init_len, np.array([max(1, s // 10) for s in range(400)], np.int32))
    want = R.search_roll(*args)
    assert want["flags"].tolist() == [0, R.WIDE] and want["jaccard"][0] > 0 and want["ref_start"][0] > 1000
    check_both(eng, args, want)


def test_member_cap_at_1024_and_one_more(eng):
    rng = np.random.default_rng(9)
    seq, r = dense_reference(rng, 5000)
    q = S.records(M.get_minimizers(seq[300:2900], 10, 1, True))
    assert len(q) > 1030
    windows = np.zeros(len(q), S.WINDOW)
    windows["n_members"], windows["query_size"] = 1, 1
    windows[0] = (len(set(R.keys_of(q[:1024]))), 1024, 0, 0, 0)
    windows[1] = (len(set(R.keys_of(q[1:1026]))), 1025, 0, 0, 0)
    first = np.zeros(len(q) + 1, np.int64)
    first[1], first[2:] = 1, 2
    intervals = np.array([(100, 500), (100, 500)], S.INTERVAL)
    args = (q, windows, first, intervals, r, len(seq), 2200, np.array([max(1, s // 4) for s in range(1100)], np.int32))
    want = R.search_roll(*args)
    assert want["flags"].tolist() == [0, R.WIDE] and want["jaccard"][0] > 0 and want["ref_start"][0] > 100
    check_both(eng, args, want)


def test_degenerate_intervals(eng):
    q = S.records([(5, 0, 0), (6, 10, 0), (5, 20, 1), (7, 30, 0)])
    r = S.records([(6, 95, 0), (5, 100, 0), (6, 110, 0), (5, 120, 2), (9, 130, 0), (7, 180, 0), (5, 190, 0), (3, 199, 0)])
    windows = np.array([(3, 4, 0, 0, 0), (1, 1, 0, 0, 0), (2, 2, 0, 0, 0), (1, 1, 0, 0, 0)], S.WINDOW)
    first = np.array([0, 3, 5, 7, 8], np.int64)
    intervals = np.array([(100, 100), (90, 140), (150, 199),   # start == end: no step; a plain one; the walk ends at len_r
                          (100, 100), (60, 130),               # query_size == 1
                          (195, 260), (199, 199),              # the first window is clamped at len_r already
                          (0, 199)], S.INTERVAL)
    args = (q, windows, first, intervals, r, 200, 20, np.array([1, 1, 2, 2], np.int32))
    want = R.search_roll(*args)
    assert (want["ref_start"][0], want["ref_end"][0]) == (100, 120) and want["ref_end"][5] == 200 and want["ref_start"][5] == 195
    assert want["ref_end"].max() <= 200 and len(set(want["jaccard"].tolist())) >= 3
    check_both(eng, args, want)


def test_empty_inputs_launch_nothing(eng):
    q, windows, first, intervals, r, len_r, init_len, limit = random_inputs(np.random.default_rng(4))
    launches = eng.last_launches()
    none = np.zeros(len(q) + 1, np.int64)
    code, got = eng.search_roll_raw(q, windows, none, intervals[:0], r, len_r, init_len, limit)  # no interval
    assert code == 0 and len(got) == 0
    code, got = eng.search_roll_raw(q[:0], windows[:0], none[:1], intervals[:0], r, len_r, init_len, limit)  # nq == 0
    assert code == 0 and len(got) == 0
    fn = eng.lib.sdf_search_roll_device
    assert fn(eng.ctx, None, 0, None, None, None, 7, None, 0, 100, 10, None, 0, None, None) == 0  # nq == 0
    assert fn(eng.ctx, 8, 5, 8, 8, 8, 0, 8, 3, 100, 10, 8, 4, None, None) == 0  # n_max == 0
    assert fn(eng.ctx, None, 5, None, None, None, 7, None, 0, 100, 10, None, 0, None, None) == SDF_ERR_INVALID
    assert eng.search_roll_raw(q, windows, first, intervals, r, len_r, 0, limit)[0] == SDF_ERR_INVALID
    assert b"init_len" in eng.lib.sdf_last_error(eng.ctx)
    assert eng.last_launches() == launches
    # ... and zero intervals on the device: every wavefront leaves at once
    got, behind = device_form(eng, q, windows, none, intervals, r, len_r, init_len, limit, n_max=9)
    assert got.tobytes() == b"\xEE" * (24 * 9) and behind == b"\xEE" * (24 * GUARD)
    assert eng.last_launches() == launches + 1
