"""Search against the SDs already found on the device: sdf_search_windows_found / _device and sdf_search_overlap / _device
(sedef_amd/csrc/search_found.hip, search_window_kernel<.., true> of search_seeds.hip).

Expected values: the host forms (sdf_search_windows_found_host, sdf_search_overlap_host) and the record-list model of
tests/found_model.py, which tests/test_search_found_cpu.py checks against the point-level model of the reference's tree.
Every comparison is exact."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch  # (at collection: before the library brings a HIP runtime of its own along)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import found_model as FM  # noqa: E402
import search_model as S  # noqa: E402
from test_search_found_cpu import (REPLAYS, host_overlap, host_windows, kwargs, overlap_arrays, overlap_scenarios, replayed,  # noqa: E402
                                   wide_case, window_scenarios)
from test_search_windows_cpu import load_fixture, same_records  # noqa: E402

pytestmark = pytest.mark.gpu

SDF_ERR_UNSUPPORTED, SDF_ERR_INVALID, SDF_ERR_OVERFLOW = -3, -4, -5
BIG = 1 << 31
CANARY = 8  # records behind every capacity, filled with 0xEE


@pytest.fixture(scope="module")
def eng():
    import sedef_amd
    e = sedef_amd.Extz2Engine(0)
    yield e
    e.close()


def ex():
    from sedef_amd import extz2
    return extz2


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def ptr(t):
    return t.data_ptr() if t.numel() else None


def raw_windows(eng, q, r, found, visible, **kw):
    code, first, windows, out, used = eng.search_windows_found_raw(q, r, found=found, visible=visible, **kw)
    assert code == 0, eng.lib.sdf_last_error(eng.ctx).decode()
    assert used == int(first[-1]) == len(out)
    return first.astype(np.int64), windows, out


def device_windows(eng, q, r, found, visible, cap, entries_cap=None, stream=None, **kw):
    """sdf_search_windows_found_device on arrays uploaded here.  Returns (code, used, first, windows, the bytes of out and of
    the canary records behind out[cap], the entries the index needed)."""
    extz2 = ex()
    limit = np.ascontiguousarray(kw["limit"], np.int32)
    found = np.ascontiguousarray(found, extz2.SEARCH_FOUND_DTYPE)
    visible = np.ascontiguousarray(visible, np.uint32)
    entries_cap = extz2.found_entries(found) if entries_cap is None else entries_cap
    d_q, d_r, d_limit, d_found, d_vis = up(q), up(r), up(limit), up(found), up(visible)
    d_first = torch.zeros(len(q) + 1, dtype=torch.int64, device="cuda")
    d_win = torch.full((len(q) * 20,), 0xEE, dtype=torch.uint8, device="cuda")
    d_out = torch.full(((cap + CANARY) * 8,), 0xEE, dtype=torch.uint8, device="cuda")
    d_need = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()  # (the tensors were filled on torch's stream)
    used = C.c_size_t(0)
    code = eng.lib.sdf_search_windows_found_device(
        eng.ctx, d_q.data_ptr(), len(q), int(kw["len_q"]), ptr(d_r), len(r), int(kw["r_threshold"]), int(kw["init_len"]),
        int(kw["same_genome"]), int(kw["uppercase_seeds"]), ptr(d_limit), len(limit), ptr(d_found), len(found), entries_cap,
        d_need.data_ptr(), d_vis.data_ptr(), d_first.data_ptr(), d_win.data_ptr(), d_out.data_ptr(), cap, C.byref(used),
        stream.cuda_stream if stream is not None else None)
    if stream is not None:
        stream.synchronize()
    windows = np.frombuffer(d_win.cpu().numpy().tobytes(), extz2.SEARCH_WINDOW_DTYPE)
    return code, int(used.value), d_first.cpu().numpy(), windows, d_out.cpu().numpy().tobytes(), int(d_need.cpu()[0])


def check_device_windows(eng, q, r, found, visible, want, stream=None, **kw):
    first, windows, out = want
    code, used, gf, gw, raw, need = device_windows(eng, q, r, found, visible, len(out), stream=stream, **kw)
    assert code == 0 and (stream is not None or used == len(out))
    assert need == (ex().found_entries(found) if len(q) else -1)  # (no query minimizer: SDF_OK without a launch, nothing written)
    same_records((gf, gw, np.frombuffer(raw[:8 * len(out)], ex().SEARCH_INTERVAL_DTYPE)), want)
    assert raw[8 * len(out):] == b"\xEE" * (8 * CANARY)


def raw_overlap(eng, q, first, rolls, found, visible_iv, init_len, mrs):
    code, out = eng.search_overlap_raw(q, first, rolls, found, visible_iv, init_len, mrs)
    assert code == 0, eng.lib.sdf_last_error(eng.ctx).decode()
    return out


def device_overlap(eng, q, first, rolls, found, visible_iv, init_len, mrs, extra=5, entries_cap=None, stream=None, d_tasks=None):
    """sdf_search_overlap_device with n_max = the intervals + extra.  Returns (code, the n_max verdicts, the canary behind them,
    the entries the index needed)."""
    extz2 = ex()
    found = np.ascontiguousarray(found, extz2.SEARCH_FOUND_DTYPE)
    n = int(first[-1])
    n_max = n + extra
    vis = np.concatenate([np.ascontiguousarray(visible_iv, np.uint32)[:n], np.full(extra, 0xFFFFFFFF, np.uint32)])
    entries_cap = extz2.found_entries(found) if entries_cap is None else entries_cap
    d_q, d_first, d_rolls, d_found, d_vis = up(q), up(np.ascontiguousarray(first, np.uint64)), up(rolls[:n]), up(found), up(vis)
    d_out = torch.full(((n_max + CANARY) * 4,), 0xEE, dtype=torch.uint8, device="cuda")
    d_need = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    code = eng.lib.sdf_search_overlap_device(eng.ctx, d_q.data_ptr(), len(q), d_first.data_ptr(), ptr(d_rolls), n_max, ptr(d_found),
                                             len(found), entries_cap, d_need.data_ptr(), d_vis.data_ptr(), init_len, mrs, d_out.data_ptr(),
                                             d_tasks, stream.cuda_stream if stream is not None else None)
    if stream is not None:
        stream.synchronize()
    raw = d_out.cpu().numpy().tobytes()
    return code, np.frombuffer(raw[:4 * n_max], np.uint32), raw[4 * n_max:], int(d_need.cpu()[0])


def check_device_overlap(eng, q, first, rolls, found, visible_iv, init_len, mrs, want, stream=None):
    code, got, canary, need = device_overlap(eng, q, first, rolls, found, visible_iv, init_len, mrs, stream=stream)
    n = int(first[-1])
    assert code == 0 and need == ex().found_entries(found)
    assert np.array_equal(got[:n], want) and not got[n:].any() and canary == b"\xEE" * (4 * CANARY)


# ---- 1. the replay ----

@pytest.mark.parametrize("which", REPLAYS)
def test_replay_through_every_form(eng, which):
    R = replayed(which)
    q, r, found, visible, kw = R["q"], R["r_sorted"], R["found"], R["visible"], R["kw"]
    want = host_windows(q, r, found, visible, **kw)
    same_records(want, (R["first"], R["windows"], R["intervals"]))
    assert len(found) >= 5 and R["lost"] >= 1 and not (want[1]["flags"] & (S.WIDE | FM.FOUND_WIDE)).any()
    same_records(raw_windows(eng, q, r, found, visible, **kw), want)
    check_device_windows(eng, q, r, found, visible, want, **kw)
    check_device_windows(eng, q, r, found, visible, want, stream=torch.cuda.Stream(), **kw)
    init_len, mrs = kw["init_len"], R["min_read_size"]
    verdicts = host_overlap(q, R["first"], R["rolls"], found, R["visible_iv"], init_len, mrs)
    assert np.array_equal(verdicts, R["verdicts"]) and verdicts.sum() >= 1
    assert np.array_equal(raw_overlap(eng, q, R["first"], R["rolls"], found, R["visible_iv"], init_len, mrs), verdicts)
    check_device_overlap(eng, q, R["first"], R["rolls"], found, R["visible_iv"], init_len, mrs, verdicts)
    check_device_overlap(eng, q, R["first"], R["rolls"], found, R["visible_iv"], init_len, mrs, verdicts, stream=torch.cuda.Stream())


# ---- 2. the empty list ----

def test_empty_list_identity_through_an_uploaded_pool(eng):
    extz2 = ex()
    some = FM.found_records([(0, 10 ** 6, 0, 10 ** 6), (5, 900, 7, 1200)])
    n_iv = 0
    for c in load_fixture()["cases"]:
        q_text = c["q"].encode()
        pool = b"gattaca" + q_text + b"NNNcat"
        q_range = r_range = (7, len(q_text))
        if not c["same"]:
            r_range = (len(pool), len(c["r"]), bool(c["r_rc"]))
            pool += c["r"].encode() + b"acgt"
        eng.pool_upload(pool)

        def one(rng):
            return eng.minim_ranges([rng[:2]], rc=bool(rng[2]) if len(rng) > 2 else None)
        _, q = eng.pool_minimizers(one(q_range), c["k"], c["w"], c["sl"])
        _, r_sorted, _, _ = eng.pool_minimizer_index(one(r_range), c["k"], c["w"], c["sl"])
        kw = dict(r_threshold=c["threshold"], len_q=len(q_text), init_len=c["init_len"], same_genome=c["same_genome"],
                  uppercase_seeds=c["uppercase_seeds"], limit=c["limit"])
        code, first, windows, out, used = eng.search_windows_raw(q, r_sorted, **kw)
        assert code == 0
        plain = (first.astype(np.int64), windows, out)
        zeros = np.zeros(len(q), np.uint32)
        same_records(raw_windows(eng, q, r_sorted, FM.found_records([]), zeros, **kw), plain)
        same_records(raw_windows(eng, q, r_sorted, some, zeros, **kw), plain)  # (the kernels with the exclusion, nothing visible)
        if not (windows["flags"] & S.WIDE).any():
            check_device_windows(eng, q, r_sorted, some, zeros, plain, **kw)
            check_device_windows(eng, q, r_sorted, some[:0], zeros, plain, **kw)
        n = int(first[-1])
        rolls = np.zeros(n, extz2.SEARCH_ROLL_DTYPE)
        rolls["ref_start"], rolls["ref_end"] = out["start"], out["start"] + c["init_len"]
        if n:
            assert not raw_overlap(eng, q, first, rolls, some, np.zeros(n, np.uint32), c["init_len"], c["init_len"]).any()
            assert not raw_overlap(eng, q, first, rolls, some[:0], np.zeros(n, np.uint32), c["init_len"], c["init_len"]).any()
        n_iv += n
    assert n_iv > 100


# ---- 3. the hand-made edges ----

def test_hand_made_window_edges(eng):
    for name, q, r, found, visible, kw, shows in window_scenarios():
        want = host_windows(q, r, found, visible, **kw)
        assert shows(want), name
        same_records(raw_windows(eng, q, r, found, visible, **kw), want)
        check_device_windows(eng, q, r, found, visible, want, **kw)


def test_hand_made_overlap_edges(eng):
    """Every scenario as one window of one call per (init_len, min_read_size), each interval with its own prefix -- and every
    scenario's records in ONE list, so that a prefix is the only thing that separates them."""
    cases = overlap_scenarios()
    for init_len, mrs in sorted({(c[5], c[6]) for c in cases}):
        mine = [c for c in cases if (c[5], c[6]) == (init_len, mrs)]
        # interval t sees its own records alone: they are moved to a query place of their own (a multiple of a bin plus the loc)
        rows, vis, moved = [], [], []
        for t, (name, loc, ref, found, v, _, _, want) in enumerate(mine):
            shift = 40960 * (t + 1)
            moved.append((name, loc + shift, ref))
            rows += [(a + shift, b + shift, c, d) for a, b, c, d in found]
            vis.append(len(rows) - len(found) + v)
        q, first, rolls = overlap_arrays(moved)
        found = FM.found_records(rows)
        want = np.array([c[7] for c in mine], np.uint32)
        assert np.array_equal(host_overlap(q, first, rolls, found, vis, init_len, mrs), want)
        assert np.array_equal(FM.search_overlap(q, first, rolls, found, vis, init_len, mrs), want)
        assert np.array_equal(raw_overlap(eng, q, first, rolls, found, vis, init_len, mrs), want)
        check_device_overlap(eng, q, first, rolls, found, vis, init_len, mrs, want)


def test_a_verdict_that_depends_on_the_intervals_own_prefix(eng):
    extz2 = ex()
    q = S.records([(7, 1000, 0), (8, 2000, 0)])
    first = np.array([0, 2, 3], np.uint64)
    rolls = np.zeros(3, extz2.SEARCH_ROLL_DTYPE)
    rolls["ref_start"], rolls["ref_end"] = [5000, 5020, 5000], [5100, 5120, 5100]
    found = FM.found_records([(900, 1200, 4900, 5200)])
    for vis, want in (([0, 1, 1], [0, 1, 0]), ([1, 0, 0], [1, 0, 0]), ([1, 1, 1], [1, 1, 0])):
        assert host_overlap(q, first, rolls, found, vis, 100, 100).tolist() == want
        assert raw_overlap(eng, q, first, rolls, found, vis, 100, 100).tolist() == want
        check_device_overlap(eng, q, first, rolls, found, vis, 100, 100, np.array(want, np.uint32))


# ---- 4. bin seams ----

def test_records_and_windows_at_the_bin_seams(eng):
    B = 1 << FM.BIN_SHIFT
    # windows at 4,000 (its span [4000, 4200] crosses the seam at 4,096), at 8,100 and 8,300 (inside bin 1 .. 2), at 9,000
    q = S.records([(1, 4000, 0), (2, 4150, 0), (3, 8100, 0), (4, 8300, 0), (5, 9000, 0)])
    r = S.index_order(S.records([(h, 100 * h + d, 0) for h in range(1, 6) for d in (0, 7)]))
    found = FM.found_records([
        (B - 50, B, 100, 101),         # ends exactly on the seam: covers 4,046 .. 4,095, not the member at 4,150
        (B, B + 100, 200, 201),        # starts exactly on it: covers the member at 4,150
        (4000, 4200, 107, 108),        # one record in both bins of window 0: staged once
        (B - 10, 3 * B + 10, 300, 308),  # spans three bins and more, the windows at 8,100 and 8,300 inside the middle ones
        (2 * B, 2 * B + 1, 407, 408),  # a single base at a seam: 8,192 is no member's loc
        (0, 10 * B, 507, 508)])        # spans every bin in play
    visible = np.full(len(q), len(found), np.uint32)
    kw = kwargs(init_len=200, len_q=10 ** 6)
    want = FM.search_windows_found(q, r, found=found, visible=visible, **kw)
    assert want[1]["n_gathered"].tolist() == [4, 2, 4, 2, 2] and want[1]["n_candidates"].tolist() == [2, 1, 2, 2, 1]
    same_records(host_windows(q, r, found, visible, **kw), want)
    same_records(raw_windows(eng, q, r, found, visible, **kw), want)
    check_device_windows(eng, q, r, found, visible, want, **kw)
    assert ex().found_entries(found) == 1 + 1 + 2 + 4 + 1 + 10
    # staged once: 251 more records that meet window 0 make 256 with the five above, three of them in both bins -- not
    # FOUND_WIDE; one more is
    fill = [(4000 + (t % 200), 4001 + (t % 200), 10 ** 6, 10 ** 6 + 1) for t in range(251)]  # (records 0, 1, 2, 3 and 5 meet it too)
    for extra, wide in ((0, False), (1, True)):
        more = FM.found_records(FM.rows_of(found) + fill + [(4096, 4097, 10 ** 6, 10 ** 6 + 1)] * extra)
        vis = np.full(len(q), len(more), np.uint32)
        want = FM.search_windows_found(q, r, found=more, visible=vis, device=True, **kw)
        assert bool(want[1]["flags"][0] & FM.FOUND_WIDE) == wide and not want[1]["flags"][1:].any()
        check_device_windows(eng, q, r, more, vis, want, **kw)
    # the overlap call walks the one bin of the window's loc: a record that starts in the bin before, one that starts on the seam
    q2 = S.records([(1, B, 0), (2, B - 1, 0), (3, 2 * B + 5, 0)])
    first = np.array([0, 1, 2, 3], np.uint64)
    rolls = np.zeros(3, ex().SEARCH_ROLL_DTYPE)
    rolls["ref_start"], rolls["ref_end"] = 5000, 5100
    found2 = FM.found_records([(B, B + 100, 5000, 5100), (B - 1, B + 99, 5000, 5100), (B - 10, 3 * B, 4000, 6000)])
    for vis, want in (([1, 1, 1], [1, 0, 0]), ([2, 2, 2], [1, 1, 0]), ([3, 3, 3], [1, 1, 1]), ([0, 3, 2], [0, 1, 0])):
        assert host_overlap(q2, first, rolls, found2, vis, 100, 100).tolist() == want
        assert raw_overlap(eng, q2, first, rolls, found2, vis, 100, 100).tolist() == want
        check_device_overlap(eng, q2, first, rolls, found2, vis, 100, 100, np.array(want, np.uint32))


# ---- 5. FOUND_WIDE ----

def test_found_wide_at_256_and_257_and_a_run_of_70(eng):
    for n in (70, 256, 257):
        q, r, found, visible, kw = wide_case(n)
        want = host_windows(q, r, found, visible, **kw)
        assert bool(want[1]["flags"][0] & FM.FOUND_WIDE) == (n > 256) and want[1]["n_candidates"].tolist() == [2, 1, 2]
        same_records(raw_windows(eng, q, r, found, visible, **kw), want)  # the stream-less form completes the window
        dev = FM.search_windows_found(q, r, found=found, visible=visible, device=True, **kw)
        if n > 256:  # the device form flags it and writes no interval for it
            assert dev[1]["n_candidates"][0] == 0 and dev[0][1] == 0 and want[0][1] > 0 and dev[1]["n_gathered"][0] == 3
        else:
            same_records(dev, want)
        check_device_windows(eng, q, r, found, visible, dev, **kw)
    # the record that decides is the last of the list (the order inside a bin is the device's: any of the 70 may be staged in the
    # second 64-lane round of the compaction)
    q, r, found, visible, kw = wide_case(70)
    rows = FM.rows_of(found)
    late = FM.found_records(rows[1:70] + [rows[0]] + rows[70:])
    want = host_windows(q, r, late, visible, **kw)
    assert want[1]["n_candidates"].tolist() == [2, 1, 2]
    check_device_windows(eng, q, r, late, visible, want, **kw)
    cut = np.array([69, 70, 70], np.uint32)  # ... and a prefix that ends in front of it
    want = host_windows(q, r, late, cut, **kw)
    assert want[1]["n_candidates"].tolist() == [3, 1, 2]
    check_device_windows(eng, q, r, late, cut, want, **kw)


# ---- 6. capacities ----

def test_capacities_at_the_need_below_it_and_zero(eng):
    extz2 = ex()
    R = replayed(REPLAYS[0])
    q, r, found, visible, kw = R["q"], R["r_sorted"], R["found"], R["visible"], R["kw"]
    want = (R["first"], R["windows"], R["intervals"])
    need = len(want[2])
    assert need > 50
    for cap in (need, need - 1, 0):
        buf = np.frombuffer(b"\xEE" * (8 * (need + 8)), extz2.SEARCH_INTERVAL_DTYPE).copy()
        code, first, windows, out, used = eng.search_windows_found_raw(q, r, found=found, visible=visible, cap=cap, out=buf, **kw)
        assert used == need and np.array_equal(first.astype(np.int64), want[0]) and windows.tobytes() == want[1].tobytes()
        if cap >= need:
            assert code == 0 and buf[:need].tobytes() == want[2].tobytes() and buf[need:].tobytes() == b"\xEE" * 64
        else:
            assert code == SDF_ERR_OVERFLOW and buf.tobytes() == b"\xEE" * (8 * (need + 8))
        code, used, gf, gw, raw, entries = device_windows(eng, q, r, found, visible, cap, **kw)
        assert used == need and np.array_equal(gf, want[0]) and raw[8 * cap:] == b"\xEE" * (8 * CANARY)
        assert code == (0 if cap >= need else SDF_ERR_OVERFLOW)
        whole = max([int(want[0][i + 1]) for i in range(len(q)) if want[0][i + 1] <= cap] + [0])
        assert raw[:8 * whole] == want[2][:whole].tobytes()
    # found_entries_cap likewise: at the need the answer, below it the code and the need, and nothing behind the intervals' cap
    entries = extz2.found_entries(found)
    assert entries >= len(found) >= 5
    for ecap in (entries, entries - 1, 0):
        code, used, gf, gw, raw, got = device_windows(eng, q, r, found, visible, need, entries_cap=ecap, **kw)
        assert got == entries and raw[8 * need:] == b"\xEE" * (8 * CANARY)
        if ecap >= entries:
            assert code == 0 and raw[:8 * need] == want[2].tobytes()
        else:
            assert code == SDF_ERR_OVERFLOW and str(entries).encode() in eng.lib.sdf_last_error(eng.ctx)
        code, verdicts, canary, got = device_overlap(eng, q, R["first"], R["rolls"], found, R["visible_iv"], kw["init_len"],
                                                     R["min_read_size"], entries_cap=ecap)
        assert got == entries and canary == b"\xEE" * (4 * CANARY)
        if ecap >= entries:
            assert code == 0 and np.array_equal(verdicts[:len(R["verdicts"])], R["verdicts"])
        else:
            assert code == SDF_ERR_OVERFLOW


# ---- 7. the skip tasks ----

def test_overlapped_intervals_are_skipped_by_the_filter_and_the_extension(eng):
    extz2 = ex()
    which = REPLAYS[1]
    R = replayed(which)
    q, found, kw = R["q"], R["found"], R["kw"]
    n, nq, init_len = int(R["first"][-1]), len(q), kw["init_len"]
    verdicts = R["verdicts"]
    assert verdicts.sum() >= 1 and n > 20
    eng.pool_upload(R["pool"])
    eng.pool_sync()
    limit = np.ascontiguousarray(kw["limit"], np.int32)
    d_q, d_win, d_first, d_iv, d_rolls, d_r, d_limit = (up(q), up(R["windows"]), up(R["first"].astype(np.uint64)), up(R["intervals"]),
                                                        up(R["rolls"]), up(R["r"]), up(limit))
    d_found, d_vis = up(found), up(R["visible_iv"])
    len_q, len_r = kw["len_q"], R["len_r"]
    stream = torch.cuda.Stream()
    eparams = extz2.extend_params(same_genome=bool(which[1]), max_sd_size=int(2.5 * init_len))

    def run(with_overlap):
        d_tasks = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
        d_frec = torch.zeros(n * 20, dtype=torch.uint8, device="cuda")
        d_hits = torch.zeros(n * 40, dtype=torch.uint8, device="cuda")
        d_out = torch.zeros(n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        s = stream.cuda_stream
        eng.search_filter_tasks_device(d_q.data_ptr(), nq, d_win.data_ptr(), d_first.data_ptr(), d_iv.data_ptr(), d_rolls.data_ptr(), n,
                                       len_q, len_r, init_len, R["q_off"], 0, R["r_off"], 0, 1, d_tasks.data_ptr(), stream=s)
        if with_overlap:
            eng.search_overlap_device(d_q.data_ptr(), nq, d_first.data_ptr(), d_rolls.data_ptr(), n, d_found.data_ptr(), len(found),
                                      extz2.found_entries(found), None, d_vis.data_ptr(), init_len, R["min_read_size"],
                                      d_out.data_ptr(), d_filter_tasks=d_tasks.data_ptr(), stream=s)
        eng.search_filter_device(d_tasks.data_ptr(), n, 0, d_frec.data_ptr(), stream=s)
        eng.search_extend_device(d_q.data_ptr(), nq, d_win.data_ptr(), d_first.data_ptr(), d_iv.data_ptr(), d_rolls.data_ptr(),
                                 d_frec.data_ptr(), n, d_r.data_ptr(), len(R["r"]), len_q, len_r, init_len, d_limit.data_ptr(), len(limit),
                                 d_hits.data_ptr(), params=eparams, stream=s)
        stream.synchronize()
        return (np.frombuffer(d_tasks.cpu().numpy().tobytes(), extz2.FILTER_TASK_DTYPE),
                np.frombuffer(d_frec.cpu().numpy().tobytes(), extz2.FILTER_REC_DTYPE),
                np.frombuffer(d_hits.cpu().numpy().tobytes(), extz2.SEARCH_HIT_DTYPE), d_out.cpu().numpy().astype(np.uint32))
    tasks0, frec0, hits0, _ = run(False)
    tasks1, frec1, hits1, out = run(True)
    assert np.array_equal(out, verdicts)
    one = verdicts == 1
    assert (hits0["flags"][one] & extz2.EXTEND_SKIPPED == 0).any()  # (without the call such an interval is extended)
    skip = np.zeros(1, extz2.FILTER_TASK_DTYPE)
    skip["flags"] = extz2.FILTER_SKIP
    assert all(t.tobytes() == skip.tobytes() for t in tasks1[one])
    assert (frec1["flags"][one] == extz2.FILTER_SKIPPED).all() and (hits1["flags"][one] == extz2.EXTEND_SKIPPED).all()
    assert tasks1[~one].tobytes() == tasks0[~one].tobytes() and frec1[~one].tobytes() == frec0[~one].tobytes()
    assert hits1[~one].tobytes() == hits0[~one].tobytes()


# ---- 8. refusals ----

def test_refusals_launch_nothing(eng):
    extz2 = ex()
    q, r = S.records([(1, 50, 0), (2, 60, 0)]), S.index_order(S.records([(1, 500, 0)]))
    found = FM.found_records([(0, 100, 4000, 6000)])
    vis = np.array([1, 1], np.uint32)
    kw = kwargs()
    assert raw_windows(eng, q, r, found, vis, **kw)[0].tolist() == [0, 1, 1]
    launches = eng.last_launches()

    def wcode(found=found, visible=vis, **change):
        return eng.search_windows_found_raw(q, r, found=found, visible=visible, **dict(kw, **change))[0]
    assert wcode(init_len=0) == SDF_ERR_INVALID and wcode(init_len=(1 << 30) + 1) == SDF_ERR_UNSUPPORTED
    assert wcode(limit=[0, 3, 0]) == SDF_ERR_UNSUPPORTED
    assert wcode(visible=np.array([1, 2], np.uint32)) == SDF_ERR_INVALID and b"prefix" in eng.lib.sdf_last_error(eng.ctx)
    many = FM.found_records([(0, 2 ** 31 - 1, 0, 10)] * 4097)
    assert wcode(found=many, visible=np.array([0, 0], np.uint32)) == SDF_ERR_UNSUPPORTED
    limit = np.array(kw["limit"], np.int32)
    first, windows, used, out4 = np.zeros(3, np.uint64), np.zeros(2, S.WINDOW), C.c_size_t(0), np.zeros(4, extz2.SEARCH_INTERVAL_DTYPE)
    good_windows = good = [eng.ctx, q.ctypes.data, 2, 10 ** 9, r.ctypes.data, 1, BIG, 100, 0, 1, limit.ctypes.data, len(limit),
                           found.ctypes.data, 1, vis.ctypes.data, first.ctypes.data, windows.ctypes.data, out4.ctypes.data, 4, C.byref(used)]
    for at in (1, 4, 10, 12, 14, 15, 16, 19):
        bad = list(good)
        bad[at] = None
        assert eng.lib.sdf_search_windows_found(*bad) == SDF_ERR_INVALID, at
    bad = list(good)
    bad[13] = 1 << 31
    assert eng.lib.sdf_search_windows_found(*bad) == SDF_ERR_UNSUPPORTED
    # the device form: its scalars and its pointers (a zeroed buffer stands for every array)
    d_zero = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    z = d_zero.data_ptr()
    dev = [eng.ctx, z, 2, 10 ** 9, z, 1, BIG, 100, 0, 1, z, 64, z, 1, 1, None, z, z, z, None, 0, None, None]
    for at, value, want in ((1, None, SDF_ERR_INVALID), (12, None, SDF_ERR_INVALID), (16, None, SDF_ERR_INVALID), (7, 0, SDF_ERR_INVALID),
                            (13, 1 << 31, SDF_ERR_UNSUPPORTED), (14, 1 << 31, SDF_ERR_UNSUPPORTED)):
        bad = list(dev)
        bad[at] = value
        assert eng.lib.sdf_search_windows_found_device(*bad) == want, at
    # the overlap call
    first2 = np.array([0, 1, 2], np.uint64)
    rolls = np.zeros(2, extz2.SEARCH_ROLL_DTYPE)
    out = np.zeros(2, np.uint32)
    good = [eng.ctx, q.ctypes.data, 2, first2.ctypes.data, rolls.ctypes.data, found.ctypes.data, 1, vis.ctypes.data, 100, 100, out.ctypes.data]
    for at in (1, 3, 4, 5, 7, 10):
        bad = list(good)
        bad[at] = None
        assert eng.lib.sdf_search_overlap(*bad) == SDF_ERR_INVALID, at
    for at, value, want in ((8, 0, SDF_ERR_INVALID), (8, (1 << 30) + 1, SDF_ERR_UNSUPPORTED), (9, -1, SDF_ERR_INVALID),
                            (6, 1 << 31, SDF_ERR_UNSUPPORTED)):
        bad = list(good)
        bad[at] = value
        assert eng.lib.sdf_search_overlap(*bad) == want, (at, value)
    over = np.array([1, 2], np.uint32)
    assert eng.lib.sdf_search_overlap(*(good[:7] + [over.ctypes.data] + good[8:])) == SDF_ERR_INVALID
    assert eng.lib.sdf_search_overlap(*(good[:5] + [many.ctypes.data, len(many)] + good[7:])) == SDF_ERR_UNSUPPORTED
    dev = [eng.ctx, z, 2, z, z, 2, z, 1, 1, None, z, 100, 100, z, None, None]
    for at, value, want in ((1, None, SDF_ERR_INVALID), (6, None, SDF_ERR_INVALID), (10, None, SDF_ERR_INVALID), (13, None, SDF_ERR_INVALID),
                            (11, 0, SDF_ERR_INVALID), (12, -1, SDF_ERR_INVALID), (7, 1 << 31, SDF_ERR_UNSUPPORTED),
                            (8, 1 << 31, SDF_ERR_UNSUPPORTED), (5, 1 << 31, SDF_ERR_UNSUPPORTED)):
        bad = list(dev)
        bad[at] = value
        assert eng.lib.sdf_search_overlap_device(*bad) == want, at
    assert eng.last_launches() == launches
    # ... and a good call launches: three for the index, the five of the count pass, the emit pass; three and one
    assert eng.lib.sdf_search_windows_found(*good_windows) == 0 and used.value == 1 and first.tolist() == [0, 1, 1]
    assert eng.last_launches() == launches + 9
    assert eng.lib.sdf_search_overlap(*good) == 0 and eng.last_launches() == launches + 13
