"""GPU: sdf_line_order and sdf_line_order_device equal the model (tests/report_model.py) on every case table of
tests/report_cases.py -- order, flags and counts (line_order.hip); SDF_LINE_WIDE on the runs of more than 64 lines and nowhere
else; a guard region around the device form's outputs; the refusals."""
import os
import sys

import numpy as np
import pytest
import torch  # (at collection: before the library brings a HIP runtime of its own along)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import report_cases as R  # noqa: E402
import report_model as M  # noqa: E402

pytestmark = pytest.mark.gpu

TABLES = R.tables()
GUARD = 64  # words in front of and behind each output


@pytest.fixture(scope="module")
def eng():
    import sedef_amd
    e = sedef_amd.Extz2Engine(0)
    yield e
    e.close()


def device_form(eng, pool, recs, pool_bytes=None):
    """The `_device` form on torch tensors -> (order, flags, (kept, wide runs, refused)); the guards around both outputs checked."""
    from sedef_amd import report
    n = len(recs)

    def up(a):
        return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda() if a.nbytes else torch.zeros(16, dtype=torch.uint8, device="cuda")
    d_pool, d_recs = up(pool), up(recs)
    d_order = torch.full((n + 2 * GUARD,), 0x6EEEEEEE, dtype=torch.int32, device="cuda")
    d_flags = torch.full((n + 2 * GUARD,), 0x6EEEEEEE, dtype=torch.int32, device="cuda")
    d_counts = torch.full((3 + 2 * GUARD,), 0x6EEEEEEE, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()  # (the tensors were filled on torch's stream)
    report.line_order_device(eng, d_pool.data_ptr(), len(pool) if pool_bytes is None else pool_bytes, d_recs.data_ptr(), n,
                             d_order.data_ptr() + 4 * GUARD, d_flags.data_ptr() + 4 * GUARD, d_counts.data_ptr() + 4 * GUARD)
    eng.pool_sync()  # (the context's stream)
    out = []
    for t, m in ((d_order, n), (d_flags, n), (d_counts, 3)):
        raw = t.cpu().numpy()
        assert (raw[:GUARD] == 0x6EEEEEEE).all() and (raw[GUARD + m:] == 0x6EEEEEEE).all()
        out.append(raw[GUARD:GUARD + m].view(np.uint32).tolist())
    return out[0], out[1], tuple(out[2])


def device_answer(lines, want):
    """What the device form leaves where the other forms answer `want`: a WIDE run in index order, flagged, without DUP."""
    order, flags, _ = (list(x) if isinstance(x, list) else x for x in want)
    p, wide_runs = 0, 0
    while p < len(order):
        hi = p + 1
        while hi < len(order) and M.key_cmp(lines[order[p]], lines[order[hi]]) == 0:
            hi += 1
        if hi - p > M.RUN:
            order[p:hi] = sorted(order[p:hi])
            flags[p:hi] = [M.WIDE] * (hi - p)
            wide_runs += 1
        p = hi
    return order, flags, (sum(1 for f in flags if not f & M.DUP), wide_runs, 0)


@pytest.mark.parametrize("name", sorted(TABLES))
def test_both_device_forms_equal_the_model(eng, name):
    from sedef_amd import report
    lines = TABLES[name]
    want = R.expected(name)
    pool, recs, plain = report.line_records(lines)
    assert plain == M.plain(lines)
    rc, order, flags, kept = report.line_order_host(pool, recs)
    assert rc == 0 and (order.tolist(), flags.tolist(), kept) == want
    order, flags, kept = report.line_order(eng, pool, recs)
    assert (order.tolist(), flags.tolist(), kept) == want
    assert R.wide_only_on_long_runs(lines, order.tolist(), flags.tolist())
    d_order, d_flags, d_counts = device_form(eng, pool, recs)
    assert (d_order, d_flags, d_counts) == device_answer(lines, want)
    assert R.wide_only_on_long_runs(lines, d_order, d_flags)


def test_wide_is_set_on_the_long_runs_alone():
    assert sum(1 for f in R.expected("run_lengths")[1] if f & M.WIDE) == 65
    assert sum(1 for f in R.expected("two_wide_runs_side_by_side")[1] if f & M.WIDE) == 136
    assert not any(f & M.WIDE for name in TABLES if name not in ("run_lengths", "run_of_65_alone", "two_wide_runs_side_by_side")
                   for f in R.expected(name)[1])


def test_a_pool_that_ends_with_its_last_line_is_not_read_beyond(eng):
    """(pool_bytes as the last line's end, not rounded to 16: the last sixteen bytes are read one by one)"""
    from sedef_amd import report
    lines = [R.padded(35, b"b"), R.padded(19, b"a"), R.padded(35, b"a"), R.padded(35, b"b")]
    pool, recs, _ = report.line_records(lines)
    end = int(recs["off"][-1]) + int(recs["len"][-1])
    assert end % 16 == 3 and end < len(pool)
    want = M.line_order(lines)
    assert device_form(eng, pool[:end].copy(), recs) == (want[0], want[1], (want[2], 0, 0))
    order, flags, kept = report.line_order(eng, pool[:end].copy(), recs)
    assert (order.tolist(), flags.tolist(), kept) == want


def test_two_calls_in_a_row_do_not_see_each_others_runs(eng):
    from sedef_amd import report
    for name in ("run_lengths", "only_k6_differs", "size_257", "three_identical_spread"):
        pool, recs, _ = report.line_records(TABLES[name])
        order, flags, kept = report.line_order(eng, pool, recs)
        assert (order.tolist(), flags.tolist(), kept) == R.expected(name)


def bad_records(recs, pool_bytes):
    """-> [(what, records)]: the last record made one the checks refuse."""
    out = []
    for what, f, v in (("off_not_a_multiple_of_16", "off", int(recs["off"][-1]) + 8), ("reserved", "reserved", 1),
                       ("past_the_pool", "len", pool_bytes - int(recs["off"][-1]) + 1), ("off_behind_the_pool", "off", pool_bytes + 16)):
        bad = recs.copy()
        bad[f][-1] = v
        out.append((what, bad))
    return out


def test_argument_errors(eng):
    from sedef_amd import report
    lines = TABLES["three_identical_spread"]
    pool, recs, _ = report.line_records(lines)
    launches = eng.last_launches()
    for what, bad in bad_records(recs, len(pool)):
        assert report.line_order_host(pool, bad)[0] == M.ERR_INVALID, what
        assert report.line_order(eng, pool, bad, check=False)[0] == M.ERR_INVALID, what
    L = report._lib()
    o, f, k = np.zeros(8, np.uint32), np.zeros(8, np.uint32), np.zeros(1, np.uint64)
    args = (pool.ctypes.data, len(pool), recs.ctypes.data, len(recs), o.ctypes.data, f.ctypes.data, k.ctypes.data)
    for hole in (0, 2, 4, 5, 6):
        holed = args[:hole] + (None,) + args[hole + 1:]
        assert L.sdf_line_order_host(*holed) == M.ERR_INVALID and L.sdf_line_order(eng.ctx, *holed) == M.ERR_INVALID
    assert L.sdf_line_order_host(*(args[:3] + ((1 << 30) + 1,) + args[4:])) == M.ERR_UNSUPPORTED
    assert report.line_order_device(eng, 256, 64, 256, (1 << 30) + 1, 256, 256, 256, check=False) == M.ERR_UNSUPPORTED
    assert report.line_order_device(eng, 256, 1 << 40, 256, 4, 256, 256, 256, check=False) == M.ERR_UNSUPPORTED
    assert report.line_order_device(eng, None, 64, 256, 4, 256, 256, 256, check=False) == M.ERR_INVALID
    assert report.line_order_device(eng, 256, 64, None, 4, 256, 256, 256, check=False) == M.ERR_INVALID
    assert report.line_order_device(eng, 256, 64, 256, 4, 256, 256, None, check=False) == M.ERR_INVALID
    assert report.line_order_device(eng, 264, 64, 256, 4, 256, 256, 256, check=False) == M.ERR_INVALID  # (a pool off the 16 bytes)
    assert eng.last_launches() == launches


def test_the_device_form_counts_what_the_host_forms_refuse_and_reads_nothing_of_it(eng):
    from sedef_amd import report
    lines = TABLES["three_identical_spread"]
    pool, recs, _ = report.line_records(lines)
    want = M.line_order(lines)
    for what, bad in bad_records(recs, len(pool)):
        order, flags, counts = device_form(eng, pool, bad)
        assert counts[2] == 1 and counts[1] == 0 and sorted(order) == list(range(len(lines))), what
        # (the refused line is the last copy of three identical ones: ordered by its keys as a line of no bytes, it leads its run)
        assert [i for i in order if i != len(lines) - 1] == [i for i in want[0] if i != len(lines) - 1], what
