"""Search seeding on the device: the reference intervals of every query window (sdf_search_windows, sdf_search_windows_device;
sedef_amd/csrc/search_seeds.hip).

Expected values: the reference's own answers (tests/golden/search_windows_kat.json.gz) and tests/search_model.py, which
tests/test_search_windows_cpu.py checks against that fixture.  Every comparison is exact: every record of first[], windows[]
and out[]."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch  # (at collection: before the library brings a HIP runtime of its own along)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import search_model as S  # noqa: E402
from test_search_windows_cpu import (case_args, case_arrays, case_expected, load_fixture, same_records,  # noqa: E402
                                     wide_arrays)

pytestmark = pytest.mark.gpu

SDF_ERR_UNSUPPORTED, SDF_ERR_INVALID, SDF_ERR_OVERFLOW = -3, -4, -5
BIG = 1 << 31


@pytest.fixture(scope="module")
def eng():
    import sedef_amd
    e = sedef_amd.Extz2Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def kat():
    return load_fixture()


def kwargs(**kw):
    base = dict(r_threshold=BIG, len_q=10 ** 9, init_len=100, same_genome=0, uppercase_seeds=1, limit=[1] * 64)
    base.update(kw)
    return base


def host_form(eng, q, r, **kw):
    code, first, windows, out, used = eng.search_windows_raw(q, r, **kw)
    assert code == 0, eng.lib.sdf_last_error(eng.ctx).decode()
    assert used == int(first[-1]) == len(out)
    return first.astype(np.int64), windows, out


def device_form(eng, q, r, cap, stream=None, **kw):
    """sdf_search_windows_device on arrays uploaded here.  Returns (code, used, first, windows, the bytes of out and of eight
    canary records behind out[cap])."""
    from sedef_amd import extz2
    limit = np.ascontiguousarray(kw["limit"], np.int32)

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    d_q, d_r, d_limit = up(q), up(r), up(limit)
    d_first = torch.zeros(len(q) + 1, dtype=torch.int64, device="cuda")
    d_win = torch.full((len(q) * 20,), 0xEE, dtype=torch.uint8, device="cuda")
    d_out = torch.full(((cap + 8) * 8,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # (the tensors were filled on torch's stream)
    used = C.c_size_t(0)
    code = eng.lib.sdf_search_windows_device(eng.ctx, d_q.data_ptr(), len(q), int(kw["len_q"]), d_r.data_ptr() if len(r) else None,
                                             len(r), int(kw["r_threshold"]), int(kw["init_len"]), int(kw["same_genome"]),
                                             int(kw["uppercase_seeds"]), d_limit.data_ptr() if len(limit) else None, len(limit),
                                             d_first.data_ptr(), d_win.data_ptr(), d_out.data_ptr(), cap, C.byref(used),
                                             stream.cuda_stream if stream is not None else None)
    if stream is not None:
        stream.synchronize()
    windows = np.frombuffer(d_win.cpu().numpy().tobytes(), extz2.SEARCH_WINDOW_DTYPE)
    return code, int(used.value), d_first.cpu().numpy(), windows, d_out.cpu().numpy().tobytes()


def check_device(eng, q, r, want, **kw):
    """The device form's answer is `want` (first, windows, intervals), with nothing written behind the intervals."""
    first, windows, out = want
    code, used, gf, gw, raw = device_form(eng, q, r, len(out), **kw)
    assert code == 0 and used == len(out)
    from sedef_amd import extz2
    same_records((gf, gw, np.frombuffer(raw[:8 * len(out)], extz2.SEARCH_INTERVAL_DTYPE)), want)
    assert raw[8 * len(out):] == b"\xEE" * 64


# ---- fixture and model agreement ----

def test_fixture_byte_for_byte_through_an_uploaded_pool(eng, kat):
    """Every case through search_windows: query and reference are different ranges of one pool (the same range for a
    same-genome case), a reversed reference lies there as the fixture has it and is named with its strand bit."""
    n_rc = 0
    for c in kat["cases"]:
        q_text = c["q"].encode()
        pool = b"gattaca" + q_text + b"NNNcat"
        q_range = (7, len(q_text))
        r_range = q_range
        if not c["same"]:
            r_range = (len(pool), len(c["r"]), bool(c["r_rc"]))
            pool += c["r"].encode() + b"acgt"
            n_rc += c["r_rc"]
        eng.pool_upload(pool)
        got = eng.search_windows(q_range, r_range, c["k"], c["w"], c["sl"], c["init_len"], c["same_genome"], c["uppercase_seeds"],
                                 c["limit"], r_threshold=c["threshold"])
        want = S.search_windows(*case_arrays(c), **case_args(c))
        same_records(got, want)
        first, out = case_expected(c)  # ... and the fixture's own numbers
        assert np.array_equal(got[0], first) and np.array_equal(np.stack([got[2]["start"], got[2]["end"]], 1), out), c["name"]
        assert got[1]["query_size"].tolist() == [w[0] for w in c["windows"]] and got[1]["flags"].tolist() == [w[1] for w in c["windows"]]
        assert got[1]["n_candidates"].tolist() == [len(w[2]) for w in c["windows"]], c["name"]
    assert n_rc >= 1


def test_random_repeat_built_sequences_against_the_model(eng):
    import minim_model as M
    rng = np.random.default_rng(3)
    letters = np.frombuffer(b"ACGT", np.uint8)
    for it, (same_genome, uppercase_seeds, init_len) in enumerate(((0, 1, 300), (1, 0, 250))):
        unit = rng.integers(0, 4, 400)

        def build(total, copies):
            parts = []
            for _ in range(copies):
                u = unit.copy()
                hit = rng.random(len(u)) < 0.03
                u[hit] = (u[hit] + 1) % 4
                parts += [rng.integers(0, 4, total // copies - 400), u]
            s = letters[np.concatenate(parts)].copy()
            s[500:640] |= 0x20
            s[900:940] = ord("N")
            return s.tobytes()
        qs = build(3000, 4)
        rs = qs if same_genome else build(3600, 5)
        q = S.records(M.closed_form_np(qs, 12, 16, True))
        r = S.index_order(S.records(M.closed_form_np(rs, 12, 16, True)))
        kw = kwargs(len_q=len(qs), init_len=init_len, same_genome=same_genome, uppercase_seeds=uppercase_seeds,
                    limit=[max(1, s // 8) for s in range(100)])
        want = S.search_windows(q, r, **kw)
        assert want[0][-1] > 100
        same_records(host_form(eng, q, r, **kw), want)
        check_device(eng, q, r, want, **kw)


# ---- hand-made edge cases: every scenario is (name, q rows, r rows, arguments, what the model's answer must show) ----

def scenarios():
    out = []

    def add(name, q_rows, r_rows, shows, **kw):
        out.append((name, S.records(q_rows), S.index_order(S.records(r_rows)), kwargs(**kw), shows))

    def intervals(ans, i=0):
        first, windows, out = ans
        return [(int(t["start"]), int(t["end"])) for t in out[first[i]:first[i + 1]]]
    # a member at exactly qs + init_len, and one a base further
    add("member at qs + init_len", [(1, 0, 0), (2, 100, 0), (3, 101, 0)], [(2, 500, 0), (3, 900, 0)],
        lambda a: a[1]["n_members"].tolist() == [2, 2, 1] and intervals(a) == [(401, 501)] and intervals(a, 1) == [(401, 501), (801, 901)])
    # qs + init_len == len_q, and one more
    add("qs + init_len at len_q", [(1, 50, 0), (1, 99, 0), (1, 100, 0), (1, 101, 0)], [(1, 7, 0)],
        lambda a: a[1]["flags"].tolist() == [0, 0, 0, S.SHORT] and a[0].tolist() == [0, 1, 2, 3, 3], len_q=200)
    # a candidate at exactly qs + init_len under same_genome, and one a base before it
    add("candidate at qs + init_len", [(1, 10, 0), (2, 11, 0)], [(1, 109, 0), (1, 110, 0), (2, 110, 0), (2, 111, 0)],
        lambda a: a[1]["n_candidates"].tolist() == [2, 1] and intervals(a) == [(110, 112)] and intervals(a, 1) == [(111, 112)],
        same_genome=1)
    add("the same without same_genome", [(1, 10, 0), (2, 11, 0)], [(1, 109, 0), (1, 110, 0), (2, 110, 0), (2, 111, 0)],
        lambda a: a[1]["n_candidates"].tolist() == [3, 2] and intervals(a) == [(10, 112)])
    # x clamped at 0
    add("x clamped at 0", [(1, 0, 0)], [(1, 0, 0), (1, 30, 0), (1, 99, 0), (1, 100, 0)],
        lambda a: intervals(a) == [(0, 101)])
    # x == last.end opens an interval, x == last.end - 1 does not (L = 1: x = c - init_len + 1, y = c + 1)
    add("x == last.end", [(1, 0, 0)], [(1, 1000, 0), (1, 1100, 0)], lambda a: intervals(a) == [(901, 1001), (1001, 1101)])
    add("x == last.end - 1", [(1, 0, 0)], [(1, 1000, 0), (1, 1099, 0)], lambda a: intervals(a) == [(901, 1100)])
    # L = 1, L = n_cand, L = n_cand + 1 (query_size 1: limit[1])
    cands = [(1, 400 + 20 * t, 0) for t in range(5)]
    add("L = 1", [(1, 0, 0)], cands, lambda a: intervals(a) == [(301, 481)], limit=[9, 1])
    add("L = n_cand", [(1, 0, 0)], cands, lambda a: a[1]["n_candidates"][0] == 5 and intervals(a) == [(381, 401)], limit=[9, 5])
    add("L = n_cand + 1", [(1, 0, 0)], cands, lambda a: a[1]["n_candidates"][0] == 5 and intervals(a) == [], limit=[9, 6])
    add("L = n_cand, too far apart", [(1, 0, 0)], cands, lambda a: intervals(a) == [], limit=[9, 5], init_len=79)
    # query_size == n_limit - 1 and == n_limit
    three = [(1, 0, 0), (2, 10, 0), (3, 20, 0), (3, 30, 0)]
    add("query_size == n_limit - 1", three, cands, lambda a: a[1]["query_size"][0] == 3 and a[1]["flags"][0] == 0 and
        len(intervals(a)) == 1, limit=[1, 1, 1, 2])
    add("query_size == n_limit", three, cands, lambda a: a[1]["query_size"][0] == 3 and a[1]["flags"][0] == S.NOLIMIT and
        a[1]["n_candidates"][0] == 5 and intervals(a) == [] and a[1]["flags"][1] == 0, limit=[1, 1, 1])
    # a group of size threshold - 1 and one of size threshold
    add("groups at the threshold", [(1, 0, 0), (2, 5, 0)], [(1, 300 + t, 0) for t in range(3)] + [(2, 900 + t, 0) for t in range(4)],
        lambda a: a[1]["n_gathered"].tolist() == [3, 0] and intervals(a) == [(201, 303)], r_threshold=4)
    # uppercase_seeds 0 and 1, with status 1 and status 2 members that have groups; all three statuses count in query_size
    mixed_q = [(5, 0, 0), (5, 10, 1), (5, 20, 2), (6, 30, 1)]
    mixed_r = [(5, 1000, 0), (5, 2000, 1), (5, 3000, 2), (6, 4000, 1), (6, 5000, 0)]
    add("uppercase seeds only", mixed_q, mixed_r, lambda a: a[1]["query_size"][0] == 4 and a[1]["n_gathered"].tolist() == [1, 0, 0, 0] and
        intervals(a) == [(901, 1001)], uppercase_seeds=1)
    add("every status seeds", mixed_q, mixed_r, lambda a: a[1]["query_size"][0] == 4 and a[1]["n_gathered"].tolist() == [4, 3, 2, 1] and
        len(intervals(a)) == 4, uppercase_seeds=0)
    # the same key three times in one window: its group is gathered three times, its candidates count once
    add("one key three times", [(7, 0, 0), (7, 40, 0), (8, 50, 0), (7, 90, 0)], [(7, 600, 0), (7, 610, 0), (8, 605, 0)],
        lambda a: a[1]["query_size"].tolist() == [2, 2, 2, 1] and a[1]["n_gathered"].tolist() == [7, 5, 3, 2] and
        a[1]["n_candidates"].tolist() == [3, 3, 3, 2] and intervals(a) == [(501, 611)])
    # no reference record at all; a hash above 2^31; locs in descending group order
    add("empty reference", [(1, 0, 0), (2, 3, 0)], [], lambda a: a[1]["n_gathered"].tolist() == [0, 0] and a[0].tolist() == [0, 0, 0])
    add("large hashes", [(0xFFFFFFFF, 0, 0), (0x80000000, 1, 0)], [(0xFFFFFFFF, 900, 0), (0x80000000, 500, 0), (0x7FFFFFFF, 100, 0)],
        lambda a: intervals(a) == [(401, 501), (801, 901)])
    return out


def test_hand_made_edge_cases(eng):
    for name, q, r, kw, shows in scenarios():
        want = S.search_windows(q, r, **kw)
        assert shows(want), (name, want)
        same_records(host_form(eng, q, r, **kw), want)
        check_device(eng, q, r, want, **kw)


# ---- seams ----

def blocks_of(gathered_counts, init_len=1000):
    """One query and one reference with a block of minimizers per count, the blocks further apart than init_len: window 0 of
    block b gathers gathered_counts[b] positions, some of them twice (wide_arrays, moved to the block's place)."""
    qs, rs, at = [], [], []
    for b, g in enumerate(gathered_counts):
        q, r = wide_arrays(g, min(40, g))
        for a in (q, r):
            a["hash"] += 1000 * b
            a["loc"] += 100000 * b
        at.append(sum(len(x) for x in qs))
        qs.append(q)
        rs.append(r)
    return np.concatenate(qs), S.index_order(np.concatenate(rs)), at


def test_gathered_counts_at_every_seam(eng):
    counts = sorted(({(1 << e) + d for e in range(13) for d in (-1, 0, 1)} | {63, 64, 65, 127, 128, 129, 5000}) - {0})
    assert {4095, 4096, 4097} <= set(counts)
    q, r, at = blocks_of(counts)
    kw = kwargs(init_len=1000, limit=[1] + [3] * 60)
    want = S.search_windows(q, r, **kw)
    assert want[1]["n_gathered"][at].tolist() == counts
    assert [bool(f & S.WIDE) for f in want[1]["flags"][at]] == [g > 4096 for g in counts]
    assert all(want[1]["n_candidates"][a] < g for a, g in zip(at, counts) if g > 50)  # (positions that come twice)
    same_records(host_form(eng, q, r, **kw), want)  # the WIDE windows of the host form equal the model
    # the device form flags them, leaves n_candidates 0 and writes nothing for them
    dev = S.search_windows(q, r, device=True, **kw)
    wide = [a for a, g in zip(at, counts) if g > 4096]
    assert len(wide) == 2 and all(dev[1]["n_candidates"][a] == 0 and dev[0][a] == dev[0][a + 1] and want[0][a] < want[0][a + 1] for a in wide)
    check_device(eng, q, r, dev, **kw)


def test_member_counts_at_the_seam(eng):
    q = S.records([(7 + (j % 3), j, j % 2) for j in range(1200)])
    r = S.index_order(S.records([(7, 50, 0), (8, 60, 0), (7, 90, 0), (9, 2000, 1), (9, 2001, 0)]))
    for init_len, members in ((1022, 1023), (1023, 1024), (1024, 1025)):
        kw = kwargs(len_q=5000, init_len=init_len, uppercase_seeds=0, limit=[1, 1, 1, 1, 1, 1, 2])
        want = S.search_windows(q, r, **kw)
        assert want[1]["n_members"][0] == members and bool(want[1]["flags"][0] & S.WIDE) == (members > 1024)
        assert want[1]["query_size"][0] == 6
        same_records(host_form(eng, q, r, **kw), want)
        check_device(eng, q, r, S.search_windows(q, r, device=True, **kw), **kw)


def test_three_thousand_windows_across_the_scan_blocks(eng):
    """first[] is a scan over 1,024 windows a round: 3,000 windows with 0 to twenty intervals each."""
    rng = np.random.default_rng(5)
    q = S.records([(int(rng.integers(0, 200)), 10 * j, 0) for j in range(3000)])
    rows = [(h, int(loc), 0) for h in range(50) for loc in rng.integers(0, 30000, int(rng.integers(1, 7)))]
    r = S.index_order(S.records(rows))
    kw = kwargs(len_q=31000, init_len=60, limit=[1] * 8 + [2] * 8)
    want = S.search_windows(q, r, **kw)
    per = np.diff(want[0])
    assert len(set(per.tolist())) >= 6 and (per == 0).sum() > 100 and 0 < want[0][1024] < want[0][2048] < want[0][3000]
    same_records(host_form(eng, q, r, **kw), want)
    check_device(eng, q, r, want, **kw)


# ---- protocol ----

def test_capacity_at_the_need_below_it_and_zero(eng):
    from sedef_amd import extz2
    q, r, at = blocks_of([5000, 300, 4100, 77])  # (two WIDE windows: the host form's need counts their intervals too)
    kw = kwargs(init_len=1000, limit=[1] + [3] * 60)
    want = S.search_windows(q, r, **kw)
    need = len(want[2])
    assert need > 100 and ((want[1]["flags"] & S.WIDE) != 0).sum() == 2
    for cap in (need - 1, need, 0):
        buf = np.frombuffer(b"\xEE" * (8 * (need + 8)), extz2.SEARCH_INTERVAL_DTYPE).copy()
        code, first, windows, out, used = eng.search_windows_raw(q, r, cap=cap, out=buf, **kw)
        assert used == need and np.array_equal(first.astype(np.int64), want[0]) and windows.tobytes() == want[1].tobytes()
        if cap >= need:
            assert code == 0 and buf[:need].tobytes() == want[2].tobytes() and buf[need:].tobytes() == b"\xEE" * 64
        else:
            assert code == SDF_ERR_OVERFLOW and buf.tobytes() == b"\xEE" * (8 * (need + 8))  # nothing is written to out
    # the device form: the need is reported, the records below cap are written and none at or behind it
    dev = S.search_windows(q, r, device=True, **kw)
    dneed = len(dev[2])
    for cap in (dneed - 1, 0):
        code, used, gf, gw, raw = device_form(eng, q, r, cap, **kw)
        assert code == SDF_ERR_OVERFLOW and used == dneed and np.array_equal(gf, dev[0]) and gw.tobytes() == dev[1].tobytes()
        assert raw[8 * cap:] == b"\xEE" * 64
        whole = 0  # the intervals of the windows that lie below cap altogether are there
        for i in range(len(q)):
            if dev[0][i + 1] <= cap:
                whole = int(dev[0][i + 1])
        assert raw[:8 * whole] == dev[2][:whole].tobytes()


def test_refusals_launch_nothing(eng):
    q, r = wide_arrays(100)
    kw = kwargs(init_len=1000, limit=[1] + [3] * 60)
    launches = eng.last_launches()

    def code(**change):
        return eng.search_windows_raw(q, r, **dict(kw, **change))[0]
    assert code(init_len=0) == SDF_ERR_INVALID and b"init_len" in eng.lib.sdf_last_error(eng.ctx)
    assert code(init_len=(1 << 30) + 1) == SDF_ERR_UNSUPPORTED
    assert code(limit=[0, 3, 0]) == SDF_ERR_UNSUPPORTED and b"limit" in eng.lib.sdf_last_error(eng.ctx)
    first, windows, used = np.zeros(len(q) + 1, np.uint64), np.zeros(len(q), S.WINDOW), C.c_size_t(0)
    limit = np.array(kw["limit"], np.int32)
    good = [eng.ctx, q.ctypes.data, len(q), 10 ** 9, r.ctypes.data, len(r), BIG, 1000, 0, 1, limit.ctypes.data, len(limit),
            first.ctypes.data, windows.ctypes.data, None, 0, C.byref(used)]
    for at in (1, 4, 10, 12, 13, 16):
        bad = list(good)
        bad[at] = None
        assert eng.lib.sdf_search_windows(*bad) == SDF_ERR_INVALID, at
    bad = list(good)
    bad[15] = 3  # cap > 0 without out
    assert eng.lib.sdf_search_windows(*bad) == SDF_ERR_INVALID
    bad = list(good)
    bad[2] = 0  # nq == 0: SDF_OK without a launch
    assert eng.lib.sdf_search_windows(*bad) == 0 and used.value == 0 and first[0] == 0
    assert eng.lib.sdf_search_windows_device(eng.ctx, None, 5, 100, None, 0, BIG, 10, 0, 1, None, 0, None, None, None, 0, None, None) == SDF_ERR_INVALID
    assert eng.last_launches() == launches
    assert eng.lib.sdf_search_windows(*good) == SDF_ERR_OVERFLOW and used.value > 0  # (cap 0: counted, not emitted)
    assert eng.last_launches() == launches + 5


def test_device_form_on_a_callers_stream_equals_the_host_form(eng, kat):
    c = next(c for c in kat["cases"] if c["name"] == "repeats 1")
    q, r = case_arrays(c)
    kw = case_args(c)
    want = host_form(eng, q, r, **kw)
    assert len(want[2]) > 100 and not (want[1]["flags"] & S.WIDE).any()
    stream = torch.cuda.Stream()
    code, used, gf, gw, raw = device_form(eng, q, r, len(want[2]), stream=stream, **kw)
    assert code == 0
    from sedef_amd import extz2
    same_records((gf, gw, np.frombuffer(raw[:8 * len(want[2])], extz2.SEARCH_INTERVAL_DTYPE)), want)
    assert raw[8 * len(want[2]):] == b"\xEE" * 64
