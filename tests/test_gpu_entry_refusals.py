"""GPU: what the range entry points answer when they refuse -- sdf_pool_range_classes, sdf_pool_fetch_ranges /
sdf_pool_fetch_plan, sdf_pool_minimizers / sdf_pool_minimizer_index, sdf_stats_columns_pairs / sdf_stats_cuts_pairs /
sdf_stats_columns_batch -- and the counted-output protocol of the cuts and the minimizers.

Every refusal is pinned whole: the return code, the complete sdf_last_error string (by equality), and that neither the
launch counter nor the resident pool moved.  The strings are literals of the library's sources.  Also pinned: the order of
the checks (the first offending record is named; inside one record the flag's refusal comes before the range's).

Shapes: a resident pool of a few hundred characters, batches of 3-6 records, three alignments of about 20 columns, k = 5 and
w = 4 -- the checks are host code, nothing larger can make them go wrong.  Helpers: those of tests/test_gpu_minimizers.py,
tests/test_gpu_pool_fetch.py and tests/test_gpu_stats_cuts.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch  # (at collection: before the library brings a HIP runtime of its own along)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cuts_model  # noqa: E402
from test_gpu_minimizers import canaries, expected as minim_expected, ranges_of  # noqa: E402
from test_gpu_pool_fetch import CANARY, fetch  # noqa: E402
from test_gpu_stats_cuts import Batch, as_lists, rev_table  # noqa: E402

pytestmark = pytest.mark.gpu

UNSUPPORTED, INVALID, OVERFLOW = -3, -4, -5
K, W = 5, 4
OUTSIDE = ": sequence range outside the resident pool (sdf_pool_upload / sdf_pool_append_fasta)"
CUTS_SCORING = "stats cuts implement |match|, |mismatch| <= 63 and |gap_open| + |gap_extend| <= 63"
M, D, I = 0, 1, 2


@pytest.fixture(scope="module")
def ctx():
    """One context whose resident pool holds three hand-made alignments and some bases behind them: (engine, batch, P)."""
    import sedef_amd
    rng = np.random.default_rng(11)
    batch = Batch(rev_table())
    for runs, a_rc, b_rc in (([(M, 20)], False, False), ([(M, 8), (D, 2), (M, 10)], True, False), ([(M, 9), (I, 3), (M, 9)], False, True)):
        a, b, runs = cuts_model.make(rng, runs)
        batch.add_strings("%d runs" % len(runs), a, b, runs, a_rc, b_rc)
    batch.put(np.frombuffer(b"ACGTacgtN", np.uint8)[rng.integers(0, 9, 170)])
    batch.finish()
    eng = sedef_amd.Extz2Engine(0)
    P = len(batch.pool)
    assert eng.pool_upload(batch.pool.tobytes()) == P and 250 < P < 400
    yield eng, batch, P
    eng.close()


def refused(eng, call, code, text):
    """call() is refused with `code` and exactly `text`; no launch is counted and the pool stays what it was."""
    launches, resident = eng.last_launches(), eng.pool_bytes()
    rc = call()
    err = eng.lib.sdf_last_error(eng.ctx).decode()
    assert (rc, err) == (code, text)
    assert eng.last_launches() == launches and eng.pool_bytes() == resident


# ---- sdf_pool_range_classes ----------------------------------------------------------------------------------------
def classes(eng, rows):
    from sedef_amd.extz2 import POOL_RANGE_DTYPE
    r = np.zeros(len(rows), POOL_RANGE_DTYPE)
    for i, row in enumerate(rows):
        r[i] = row
    return eng.pool_range_classes(r, check=False)


def test_pool_range_classes(ctx):
    eng, _, P = ctx
    who = "sdf_pool_range_classes: "
    ok = (10, 50, 0)
    refused(eng, lambda: classes(eng, [ok, (10, 50, 1)])[0], UNSUPPORTED, who + "reserved must be 0")
    for bad in ((-1, 4, 0), (0, -1, 0), (P + 1, 0, 0), (P - 3, 4, 0)):
        for rows in ([bad], [ok, bad, ok]):
            refused(eng, lambda: classes(eng, rows)[0], INVALID, who + "range outside the resident pool")
    # order: the first offending record decides; inside a record `reserved` is looked at before the range
    refused(eng, lambda: classes(eng, [ok, (P - 3, 4, 0), (10, 50, 1)])[0], INVALID, who + "range outside the resident pool")
    refused(eng, lambda: classes(eng, [ok, (10, 50, 1), (P - 3, 4, 0)])[0], UNSUPPORTED, who + "reserved must be 0")
    refused(eng, lambda: classes(eng, [ok, (P - 3, 4, 7)])[0], UNSUPPORTED, who + "reserved must be 0")
    # accepted: the empty range at the pool's end, and no range at all
    from sedef_amd.extz2 import POOL_RANGE_DTYPE, RANGE_CLASSES_DTYPE
    r = np.zeros(1, POOL_RANGE_DTYPE)
    r[0] = (P, 0, 0)
    out = np.full(1, 0x5A5A5A5A, np.int32).repeat(4).view(RANGE_CLASSES_DTYPE)
    assert eng.lib.sdf_pool_range_classes(eng.ctx, r.ctypes.data, 1, out.ctypes.data) == 0
    assert not out.view(np.int32).any() and eng.lib.sdf_last_error(eng.ctx).decode() == ""
    rc, out, err = classes(eng, [])
    assert rc == 0 and err == "" and len(out) == 0
    rc, out, err = classes(eng, [ok, (P, 0, 0)])
    assert rc == 0 and sum(int(out[f][0]) for f in out.dtype.names) == 50 and not out[1:].view(np.int32).any()


# ---- sdf_pool_fetch_ranges / sdf_pool_fetch_plan -------------------------------------------------------------------
def fetch_records(rows):
    """rows: (off, len, flags, dst_off), the flag word as it is."""
    from sedef_amd.extz2 import POOL_FETCH_DTYPE
    r = np.zeros(len(rows), POOL_FETCH_DTYPE)
    for i, row in enumerate(rows):
        r[i] = row
    return r


def test_pool_fetch(ctx):
    eng, batch, P = ctx
    size = 256
    ok = (10, 100, 1, 0)

    def both(rows, code, index, why):
        r = fetch_records(rows)
        buf = np.full(size, CANARY, np.uint8)
        refused(eng, lambda: eng.lib.sdf_pool_fetch_ranges(eng.ctx, r.ctypes.data, len(r), buf.ctypes.data, size), code,
                "sdf_pool_fetch_ranges: range %d: %s" % (index, why))
        assert (buf == CANARY).all()
        plan = eng.pool_fetch_plan(r, dst_bytes=size)  # (the same checks without a context: the code and *bad)
        assert (plan[0], plan[5]) == (code, index) and plan[2:5] == (0, 0, 0)

    for flags in (2, 3, 0x100, -2147483648):
        both([ok, (10, 100, 0, 100), (10, 50, flags, 200)], UNSUPPORTED, 2, "unknown flag")
    for bad in ((-1, 4, 0, 200), (0, -1, 0, 200), (P + 1, 0, 0, 200), (P - 3, 4, 1, 200)):
        both([bad], INVALID, 0, "outside the resident pool")
        both([ok, bad, ok], INVALID, 1, "outside the resident pool")
    for bad in ((0, 4, 0, -1), (0, 4, 1, size - 3), (0, 0, 0, size + 1)):
        both([bad], INVALID, 0, "destination outside dst")
        both([ok, (0, 0, 0, size), bad], INVALID, 2, "destination outside dst")
    # order: the first offending record; inside a record the flag, then the source, then the destination
    both([ok, (P - 3, 4, 0, 200), (10, 50, 2, 200)], INVALID, 1, "outside the resident pool")
    both([ok, (10, 50, 2, 200), (P - 3, 4, 0, 200)], UNSUPPORTED, 1, "unknown flag")
    both([ok, (P - 3, 4, 2, size)], UNSUPPORTED, 1, "unknown flag")
    both([ok, (P - 3, 4, 0, size)], INVALID, 1, "outside the resident pool")
    # bytes to write and nowhere to write them: the first range that has one is named
    r = fetch_records([(0, 0, 0, 0), (10, 100, 0, 0), (10, 100, 0, 100)])
    refused(eng, lambda: eng.lib.sdf_pool_fetch_ranges(eng.ctx, r.ctypes.data, 3, None, size), INVALID,
            "sdf_pool_fetch_ranges: range 1: a byte to write and no dst")
    refused(eng, lambda: eng.lib.sdf_pool_fetch_ranges(eng.ctx, None, 1, None, size), INVALID, "sdf_pool_fetch_ranges: invalid arguments")
    # the context serves a correct call afterwards (tests/test_gpu_pool_fetch.py: fetch)
    got = fetch(eng, [(10, 100, False, 0), (P - 3, 3, False, 100)], size)
    assert got[64:164].tobytes() == batch.pool[10:110].tobytes() and got[164:167].tobytes() == batch.pool[P - 3:].tobytes()


# ---- sdf_pool_minimizers / sdf_pool_minimizer_index ----------------------------------------------------------------
@pytest.mark.parametrize("index", [False, True], ids=["sdf_pool_minimizers", "sdf_pool_minimizer_index"])
def test_minimizers(ctx, index):
    eng, batch, P = ctx
    who = "sdf_pool_minimizer_index" if index else "sdf_pool_minimizers"
    ok = (10, 100, False)

    def call(rows, k=K, w=W, flags=None):
        r = ranges_of(rows)
        for i, f in (flags or {}).items():
            r["flags"][i] = f
        out = canaries(64)
        rc = eng.pool_minimizers_raw(r, k, w, True, cap=64, out=out, index=index)[0]
        assert out.tobytes() == canaries(64).tobytes()
        return rc

    for w in (0, -1):
        refused(eng, lambda: call([ok], w=w), INVALID, "minimizers: w < 1")
    for k, w in ((0, W), (16, W), (K, 1001)):
        refused(eng, lambda: call([ok], k=k, w=w), UNSUPPORTED, "minimizers implement k 1..15 and w up to 1000")
    for f in (2, 3, 0x100, -2147483648):
        refused(eng, lambda: call([ok, ok, ok], flags={2: f}), UNSUPPORTED, "minimizers: range 2: unknown flag")
    for bad in ((-1, 4, False), (0, -1, False), (P + 1, 0, False), (P - 3, 4, True)):
        refused(eng, lambda: call([bad]), INVALID, "minimizers: range 0: outside the resident pool")
        refused(eng, lambda: call([ok, bad, ok]), INVALID, "minimizers: range 1: outside the resident pool")
    # order: the scalars before the ranges; the first offending record; inside a record the flag before the range
    refused(eng, lambda: call([(P - 3, 4, False)], w=0), INVALID, "minimizers: w < 1")
    refused(eng, lambda: call([(P - 3, 4, False)], k=16), UNSUPPORTED, "minimizers implement k 1..15 and w up to 1000")
    refused(eng, lambda: call([ok, (P - 3, 4, False), ok], flags={2: 2}), INVALID, "minimizers: range 1: outside the resident pool")
    refused(eng, lambda: call([ok, ok, (P - 3, 4, False)], flags={1: 2}), UNSUPPORTED, "minimizers: range 1: unknown flag")
    refused(eng, lambda: call([ok, (P - 3, 4, False)], flags={1: 2}), UNSUPPORTED, "minimizers: range 1: unknown flag")

    # the raw call: a null `first`, and no range at all
    def raw(n, first):
        r = ranges_of([ok])
        out, used = canaries(8), C.c_size_t(12345)
        ng, thr = np.zeros(1, np.uint32), np.zeros(1, np.uint32)
        head = (eng.ctx, r.ctypes.data, n, K, W, 1, None if first is None else first.ctypes.data, out.ctypes.data, 8, C.byref(used))
        rc = eng.lib.sdf_pool_minimizer_index(*head, ng.ctypes.data, thr.ctypes.data) if index else eng.lib.sdf_pool_minimizers(*head)
        return rc, int(used.value)

    refused(eng, lambda: raw(1, None)[0], INVALID, who + ": invalid arguments")
    first = np.full(2, 77, np.uint64)
    launches = eng.last_launches()
    assert raw(0, first) == (0, 0) and first.tolist() == [0, 77] and eng.last_launches() == launches
    assert eng.lib.sdf_last_error(eng.ctx).decode() == ""


# ---- sdf_stats_columns_pairs / sdf_stats_cuts_pairs / sdf_stats_columns_batch --------------------------------------
def stats_call(eng, form, tasks, cig, pool=None, scores=cuts_model.DEFAULT):
    """The raw call of one of the three forms; returns its code."""
    from sedef_amd.extz2 import STATS_COLS_DTYPE
    if form == "cuts":
        return eng.stats_cuts_pairs_raw(tasks, cig, scores=scores)[0]
    out = np.zeros(len(tasks), STATS_COLS_DTYPE)
    if form == "pairs":
        return eng.lib.sdf_stats_columns_pairs(eng.ctx, tasks.ctypes.data, len(tasks), cig.ctypes.data, len(cig), out.ctypes.data)
    return eng.lib.sdf_stats_columns_batch(eng.ctx, tasks.ctypes.data, len(tasks), pool, len(pool), cig.ctypes.data, len(cig),
                                           out.ctypes.data)


def changed(tasks, *edits):
    t = tasks.copy()
    for i, field, value in edits:
        t[field][i] = value
    return t


@pytest.mark.parametrize("form", ["pairs", "cuts"])
def test_stats_on_the_resident_pool(ctx, form):
    eng, batch, P = ctx
    tasks, cig = batch.tasks, batch.cig
    noun = "cuts" if form == "cuts" else "columns"
    past = lambda i, side: P - int(tasks[side + "_len"][i]) + 1  # noqa: E731  (the first offset whose range leaves the pool)

    def check(t, code, text, **kw):
        refused(eng, lambda: stats_call(eng, form, t, cig, **kw), code, text)

    for bits in (0x4, 0x80000000, 0x7):
        check(changed(tasks, (2, "reserved", bits)), UNSUPPORTED, "alignment 2: unknown stats task flag")
    for side in "ab":
        check(changed(tasks, (1, side + "_len", (1 << 24) + 1)), UNSUPPORTED, "stats %s implement sequences up to 16 Mb" % noun)
        check(changed(tasks, (1, side + "_off", past(1, side))), INVALID, "alignment 1" + OUTSIDE)
        check(changed(tasks, (0, side + "_off", P + 1), (0, side + "_len", 0)), INVALID, "alignment 0" + OUTSIDE)
    check(changed(tasks, (2, "cigar_off", len(cig) - int(tasks["n_cigar"][2]) + 1)), INVALID, "alignment 2: CIGAR range outside its pool")
    check(changed(tasks, (0, "cigar_off", len(cig) + 1), (0, "n_cigar", 0)), INVALID, "alignment 0: CIGAR range outside its pool")
    # order: the first offending record; inside a record the flag, the length, the sequence range, the CIGAR range
    check(changed(tasks, (1, "a_off", past(1, "a")), (2, "reserved", 0x4)), INVALID, "alignment 1" + OUTSIDE)
    check(changed(tasks, (1, "reserved", 0x4), (2, "a_off", past(2, "a"))), UNSUPPORTED, "alignment 1: unknown stats task flag")
    check(changed(tasks, (1, "reserved", 0x4), (1, "a_off", past(1, "a"))), UNSUPPORTED, "alignment 1: unknown stats task flag")
    check(changed(tasks, (1, "reserved", 0x4), (1, "a_len", (1 << 24) + 1)), UNSUPPORTED, "alignment 1: unknown stats task flag")
    check(changed(tasks, (1, "b_len", (1 << 24) + 1), (1, "a_off", P + 1)), UNSUPPORTED, "stats %s implement sequences up to 16 Mb" % noun)
    check(changed(tasks, (1, "b_off", past(1, "b")), (1, "cigar_off", len(cig) + 1)), INVALID, "alignment 1" + OUTSIDE)
    if form == "cuts":  # the scores are looked at before any task
        for scores in ((64, -4, -40, -1), (5, -64, -40, -1), (5, -4, -40, -24)):
            check(tasks, UNSUPPORTED, CUTS_SCORING, scores=scores)
        check(changed(tasks, (0, "reserved", 0x4)), UNSUPPORTED, CUTS_SCORING, scores=(64, -4, -40, -1))
    # the context serves a correct call afterwards
    assert stats_call(eng, form, tasks, cig) == 0 and eng.lib.sdf_last_error(eng.ctx).decode() == ""


def test_stats_columns_batch(ctx):
    eng, batch, P = ctx
    tasks, cig, pool = changed(batch.tasks), batch.cig, batch.pool.tobytes()
    tasks["reserved"] = 0x4  # (this form does not look at the word)
    either = ": sequence or CIGAR range outside its pool"

    def check(t, code, text):
        refused(eng, lambda: stats_call(eng, "batch", t, cig, pool=pool), code, text)

    for side in "ab":
        check(changed(tasks, (1, side + "_len", (1 << 24) + 1)), UNSUPPORTED, "stats columns implement sequences up to 16 Mb")
        check(changed(tasks, (1, side + "_off", P - int(tasks[side + "_len"][1]) + 1)), INVALID, "alignment 1" + either)
    check(changed(tasks, (2, "cigar_off", len(cig) - int(tasks["n_cigar"][2]) + 1)), INVALID, "alignment 2" + either)
    check(changed(tasks, (1, "a_off", P + 1), (2, "a_len", (1 << 24) + 1)), INVALID, "alignment 1" + either)
    check(changed(tasks, (1, "a_len", (1 << 24) + 1), (1, "a_off", P + 1)), UNSUPPORTED, "stats columns implement sequences up to 16 Mb")
    assert stats_call(eng, "batch", tasks, cig, pool=pool) == 0 and eng.lib.sdf_last_error(eng.ctx).decode() == ""


# ---- counted output: a capacity one short of the need ----------------------------------------------------------------
def on_device(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


def test_cuts_counted_output(ctx):
    from sedef_amd.extz2 import STATS_PIECE_DTYPE
    eng, batch, P = ctx
    tasks, cig, n = batch.tasks, batch.cig, len(batch.tasks)
    exp = batch.expected()
    need = sum(len(r) for r in exp)
    text = "the batch cuts into %d pieces, more than pieces_cap" % need
    rc, first, pieces, used = eng.stats_cuts_pairs_raw(tasks, cig)
    assert rc == 0 and used == need >= n and as_lists(first, pieces) == exp
    # the host form
    buf = np.zeros(need, STATS_PIECE_DTYPE)
    buf.view(np.int32)[:] = 0x5A5A5A5A
    rc, first2, _, used = eng.stats_cuts_pairs_raw(tasks, cig, cap=need - 1, pieces=buf)
    assert (rc, used, eng.lib.sdf_last_error(eng.ctx).decode()) == (OVERFLOW, need, text)
    assert (first2 == first).all() and (buf.view(np.int32) == 0x5A5A5A5A).all()
    assert as_lists(*eng.stats_cuts_pairs(tasks, cig)) == exp
    # the device form on the context's own stream
    d_tasks, d_cig = on_device(tasks), on_device(cig)

    def device(cap):
        d_first = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
        d_out = torch.full((need * 8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()  # (the tensors were filled on torch's stream)
        eng.pool_sync()
        used = C.c_size_t(12345)
        rc = eng.lib.sdf_stats_cuts_pairs_device(eng.ctx, d_tasks.data_ptr(), n, 1, d_cig.data_ptr(), *cuts_model.DEFAULT,
                                                 d_first.data_ptr(), d_out.data_ptr(), cap, C.byref(used), None)
        return rc, int(used.value), eng.lib.sdf_last_error(eng.ctx).decode(), d_first.cpu().numpy(), d_out.cpu().numpy()

    rc, used, err, d_first, out = device(need - 1)
    assert (rc, used, err) == (OVERFLOW, need, text) and (d_first == first.astype(np.int64)).all()
    assert (out[8 * (need - 1):] == 0x5A5A5A5A).all()
    rc, used, err, d_first, out = device(need)
    assert (rc, used, err) == (0, need, "") and (d_first == first.astype(np.int64)).all()
    assert out.view(STATS_PIECE_DTYPE).tobytes() == pieces[:need].tobytes()


def test_minimizers_counted_output(ctx):
    eng, batch, P = ctx
    rows = [(0, 120, False), (50, 0, False), (100, P - 100, True), (P - 4, 4, False)]
    wf, wr = minim_expected(batch.pool, rows, K, W, True)
    need, n = len(wr), len(rows)
    assert need > 20
    text = "the ranges have %d minimizers, more than cap" % need
    r = ranges_of(rows)
    # the host forms
    for index in (False, True):
        buf = canaries(need)
        res = eng.pool_minimizers_raw(r, K, W, True, cap=need - 1, out=buf, index=index)
        assert (res[0], res[3], eng.lib.sdf_last_error(eng.ctx).decode()) == (OVERFLOW, need, text)
        assert np.array_equal(res[1].astype(np.int64), wf) and buf.tobytes() == canaries(need).tobytes()
        res = eng.pool_minimizers_raw(r, K, W, True, cap=need, out=buf, index=index)
        assert (res[0], res[3]) == (0, need) and np.array_equal(res[1].astype(np.int64), wf)
        if not index:
            assert buf.tobytes() == wr.tobytes()
    # the device form on the context's own stream
    d_ranges = on_device(r)

    def device(cap):
        d_first = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
        d_out = torch.full((need * 16,), 0xEE, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()  # (the tensors were filled on torch's stream)
        eng.pool_sync()
        used = C.c_size_t(12345)
        rc = eng.lib.sdf_pool_minimizers_device(eng.ctx, d_ranges.data_ptr(), n, 1, K, W, 1, d_first.data_ptr(), d_out.data_ptr(), cap,
                                                C.byref(used), None)
        return rc, int(used.value), eng.lib.sdf_last_error(eng.ctx).decode(), d_first.cpu().numpy(), d_out.cpu().numpy()

    rc, used, err, d_first, out = device(need - 1)
    assert (rc, used, err) == (OVERFLOW, need, text) and np.array_equal(d_first, wf)
    assert out[:16 * (need - 1)].tobytes() == wr[:-1].tobytes() and (out[16 * (need - 1):] == 0xEE).all()
    rc, used, err, d_first, out = device(need)
    assert (rc, used, err) == (0, need, "") and np.array_equal(d_first, wf) and out.tobytes() == wr.tobytes()
