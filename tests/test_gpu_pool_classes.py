"""Character classes of ranges of the resident pool on the GPU (sdf_pool_range_classes; seq_pack.hip: pool_classes_kernel).

The expected counts are numpy's on the same bytes, compared exactly.  The class of a byte is decided on the whole byte, as the
table of the stage driver's PairJob does (sedef_amd/csrc/host/pair_job.cc): ACGT, acgt, N or n, everything else -- a byte of 128
or more is `other`."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu

SEG = 16384  # kClassSegBytes (sedef_amd/csrc/sdf_kernels.h): the bytes one group of sixteen lanes counts
POOL_LEN = 70000
SDF_ERR_UNSUPPORTED, SDF_ERR_INVALID = -3, -4

CLASS = np.full(256, 3, np.int64)  # 0 upper_acgt, 1 lower_acgt, 2 n_any, 3 other
CLASS[list(b"ACGT")] = 0
CLASS[list(b"acgt")] = 1
CLASS[list(b"Nn")] = 2


def expected(pool, ranges):
    """(n, 4) counts of the ranges' bytes, by numpy."""
    cls = CLASS[pool]
    out = np.zeros((len(ranges), 4), np.int64)
    for i, (off, ln) in enumerate(ranges):
        out[i] = np.bincount(cls[off:off + ln], minlength=4)
    return out


def as_rows(rec):
    return np.stack([rec[f].astype(np.int64) for f in ("upper_acgt", "lower_acgt", "n_any", "other")], axis=1)


def make_pool():
    rng = np.random.default_rng(20240607)
    pool = np.frombuffer(b"ACGTacgtNn", np.uint8)[rng.integers(0, 10, POOL_LEN)].copy()
    # a sprinkling of every byte value, at random places ...
    where = rng.choice(POOL_LEN, 4 * 256, replace=False)
    pool[where] = np.tile(np.arange(256, dtype=np.uint8), 4)
    # ... and the named ones at places the edge ranges below are sure to cover
    for k, c in enumerate((ord("\n"), ord("R"), ord("-"), 127, 128, 255)):
        pool[3 + 5 * k] = c
        pool[POOL_LEN - 2 - 3 * k] = c
        pool[SEG - 1 + k] = c
    for c in (ord("\n"), ord("R"), ord("-"), 127, 128, 255):
        assert (pool == c).sum() >= 4
    return pool


def edge_ranges():
    r = []
    for start in range(0, 17):
        for ln in (0, 1, 15, 16, 17, 63, 64, 65):
            r.append((start, ln))
        for ln in (SEG - 1, SEG, SEG + 1, 2 * SEG + 5):
            r.append((start, ln))
    r.append((0, 1))                                  # starts at byte 0
    for ln in (1, 15, 16, 17, 65, SEG + 1, 2 * SEG + 5):
        r.append((POOL_LEN - ln, ln))                 # ends at the pool's last byte
    r.append((POOL_LEN, 0))                           # nothing, behind the last byte
    r.append((0, POOL_LEN))                           # the whole pool
    r.append((7, POOL_LEN - 7 - 9))
    return r


@pytest.fixture(scope="module")
def resident():
    import sedef_amd
    eng = sedef_amd.Extz2Engine(0)
    pool = make_pool()
    assert eng.pool_upload(pool.tobytes()) == POOL_LEN
    yield eng, pool
    eng.close()


def test_range_edges_against_numpy(resident):
    eng, pool = resident
    ranges = edge_ranges()
    got = as_rows(eng.pool_range_classes(ranges))
    exp = expected(pool, ranges)
    bad = np.flatnonzero((got != exp).any(axis=1))
    assert len(bad) == 0, [(ranges[i], got[i].tolist(), exp[i].tolist()) for i in bad[:5]]
    assert (got.sum(axis=1) == np.array([ln for _, ln in ranges])).all()
    # the sprinkled bytes were really counted as `other` somewhere, bytes of 128 and more among them
    whole = got[ranges.index((0, POOL_LEN))]
    assert whole[3] == int((CLASS[pool] == 3).sum()) >= 900 and (pool >= 128).sum() >= 500


def test_order_and_repeats_do_not_matter(resident):
    """The records are zeroed in front of every launch and added to atomically: the same ranges backwards, and every range
    twice in one call, give the same counts."""
    eng, pool = resident
    ranges = edge_ranges()
    exp = expected(pool, ranges)
    assert (as_rows(eng.pool_range_classes(ranges[::-1])) == exp[::-1]).all()
    twice = as_rows(eng.pool_range_classes(ranges + ranges))
    assert (twice == np.concatenate([exp, exp])).all()
    # a second call on the context after a larger one: nothing of the larger call's records shows
    assert (as_rows(eng.pool_range_classes(ranges[:3])) == exp[:3]).all()


def test_appended_fasta_counts_no_line_ends():
    """Three records as a file has them -- different line lengths, a short last line, a last line without a line end -- go in
    through sdf_pool_append_fasta; ranges across what were line ends count no `other` for the '\\n'."""
    import sedef_amd
    rng = np.random.default_rng(5)
    eng = sedef_amd.Extz2Engine(0)
    try:
        recs, bases = [], []
        for n_bases, line, end in ((1000, 60, b"\n"), (777, 50, b"\r\n"), (333, 70, b"\n")):
            b = np.frombuffer(b"ACGTacgtNn", np.uint8)[rng.integers(0, 10, n_bases)].tobytes()
            lines = [b[i:i + line] for i in range(0, n_bases, line)]
            assert len(lines[-1]) < line  # a short last line
            raw = end.join(lines) + (end if len(recs) < 2 else b"")  # the third record's last line has no line end
            recs.append((raw, n_bases, line, line + len(end)))
            bases.append(b)
        offs = []
        for k, (raw, n_bases, lb, lby) in enumerate(recs):
            offs.append(eng.pool_append_fasta(raw, n_bases, lb, lby, reset=(k == 0)))
        assert offs == [0, 1000, 1777] and eng.pool_bytes() == 2110
        pool = np.frombuffer(b"".join(bases), np.uint8)
        ranges = [(0, 2110), (0, 1000), (1000, 777), (1777, 333), (55, 10), (59, 2), (1000 + 45, 10), (1777 + 60, 20),
                  (990, 30), (2110 - 1, 1)]
        got = as_rows(eng.pool_range_classes(ranges))
        assert (got == expected(pool, ranges)).all()
        assert (got[:, 3] == 0).all()
    finally:
        eng.close()


def test_contract(resident):
    from sedef_amd.extz2 import POOL_RANGE_DTYPE
    eng, pool = resident

    def call(rows):
        r = np.zeros(len(rows), POOL_RANGE_DTYPE)
        for i, row in enumerate(rows):
            r[i] = row
        return eng.pool_range_classes(r, check=False)

    ok = (10, 100, 0)
    # a range outside the pool, wherever it stands among good ones
    for bad in ((POOL_LEN, 1, 0), (POOL_LEN - 5, 6, 0), (-1, 4, 0), (POOL_LEN + 1, 0, 0), (0, POOL_LEN + 1, 0),
                (1 << 40, 5, 0)):
        for rows in ([bad], [ok, bad], [bad, ok]):
            rc, _, err = call(rows)
            assert rc == SDF_ERR_INVALID and "outside" in err, (bad, rc, err)
    rc, _, err = call([ok, (0, -1, 0)])
    assert rc == SDF_ERR_INVALID
    rc, _, err = call([ok, (0, 5, 1)])
    assert rc == SDF_ERR_UNSUPPORTED and "reserved" in err
    # len == 0 is legal everywhere up to the pool's end; n == 0 with NULL pointers is SDF_OK
    rc, out, _ = call([(0, 0, 0), (POOL_LEN, 0, 0), ok])
    assert rc == 0 and as_rows(out)[:2].sum() == 0 and (as_rows(out)[2] == expected(pool, [(10, 100)])[0]).all()
    rc, out, _ = call([(5, 0, 0)])
    assert rc == 0 and as_rows(out).sum() == 0
    assert eng.lib.sdf_pool_range_classes(eng.ctx, None, 0, None) == 0
    # pointers missing with n != 0
    assert eng.lib.sdf_pool_range_classes(eng.ctx, None, 1, None) == SDF_ERR_INVALID
    # the failed calls left the context usable
    assert (as_rows(eng.pool_range_classes([(10, 100)])) == expected(pool, [(10, 100)])).all()


def test_empty_pool_holds_no_range():
    import sedef_amd
    eng = sedef_amd.Extz2Engine(0)
    try:
        assert eng.pool_bytes() == 0
        rc, _, _ = eng.pool_range_classes([(0, 1)], check=False)
        assert rc == SDF_ERR_INVALID
        rc, out, _ = eng.pool_range_classes([(0, 0)], check=False)
        assert rc == 0 and as_rows(out).sum() == 0
        assert eng.lib.sdf_pool_range_classes(eng.ctx, None, 0, None) == 0
    finally:
        eng.close()
