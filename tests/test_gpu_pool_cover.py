"""GPU: Extz2Engine.pool_coverage (sdf_pool_coverage; pool_cover.hip) equals the definition-level model (cover_model.py) AND
sdf_pool_coverage_host, counter for counter, with `upper` and `painted` -- on sixteen regions at every pool offset residue mod 16,
of the lengths at which a word, a wavefront of words or a piece of the first two launches ends (cover_cases.py)."""
import gc
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (at collection: before the library brings a HIP runtime of its own along)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cover_cases  # noqa: E402
import cover_model  # noqa: E402

pytestmark = pytest.mark.gpu

SDF_ERR_UNSUPPORTED, SDF_ERR_INVALID = -3, -4


@pytest.fixture(scope="module")
def setup():
    """One context with the pool resident; the pool's characters for the model and the host form."""
    import sedef_amd
    records, regions = cover_cases.build_pool()
    eng = sedef_amd.Extz2Engine(0)
    offs = cover_cases.upload(eng, records)
    chars = np.concatenate(records).tobytes()
    assert eng.pool_bytes() == len(chars) and [offs[i] for i in range(len(offs))] == np.cumsum([0] + [len(r) for r in records])[:-1].tolist()
    yield eng, chars, regions
    eng.close()


def check(setup, regions, iv, min_upper):
    from sedef_amd import extz2
    eng, chars, _ = setup
    counts, upper, painted = eng.pool_coverage(regions, iv, min_upper)
    exp_counts, exp_upper, exp_painted = cover_model.coverage(chars, regions, iv, min_upper)
    rc, (h_counts, h_upper, h_painted) = extz2.pool_coverage_host(chars, regions, iv, min_upper)
    assert rc == 0
    got = cover_model.counts_rows(counts)
    bad = np.nonzero((got != exp_counts).any(axis=1))[0]
    assert len(bad) == 0, (bad[:4].tolist(), got[bad[:4]].tolist(), exp_counts[bad[:4]].tolist())
    assert (got == cover_model.counts_rows(h_counts)).all()
    assert (upper == exp_upper).all() and (upper == h_upper).all()
    assert (painted == exp_painted).all() and (painted == h_painted).all()
    return exp_counts, upper, painted


def test_edges_then_whole_then_edges(setup):
    """Word and piece edges, shared words, nested / identical / touching intervals, len == 0 -- and two calls in a row on one
    context: the bitmaps of a call do not show in the next."""
    _, _, regions = setup
    whole = check(setup, regions, cover_cases.whole_case(regions), 100)[0]
    assert [int(x) for x in whole[:, 0] + whole[:, 1]] == [n + 1 for _, n in regions]
    edges, _, painted = check(setup, regions, cover_cases.edge_case(regions), 100)
    assert painted.all() and (edges[:, 3] > 0).any() and (edges[:, 4] > 0).any() and (edges[:, 2] > 0).any()
    empty = check(setup, regions, [], 100)[0]
    assert not empty.any()


def test_partner_thresholds(setup):
    _, _, regions = setup
    iv, up, pa = cover_cases.partner_case()
    _, upper, painted = check(setup, regions, iv, 100)
    assert upper.tolist() == up and painted.tolist() == pa
    assert check(setup, regions, iv, 99)[2].all()


@pytest.mark.parametrize("seed", [1, 2])
def test_random_intervals(setup, seed):
    _, _, regions = setup
    check(setup, regions, cover_cases.random_case(regions, seed), 40)


def test_overlapping_and_unaligned_regions(setup):
    """Regions that overlap each other and that start anywhere: bitmaps of their own, each from a word boundary of its own."""
    _, chars, _ = setup
    n = len(chars)
    regions = [(off, 4000) for off in range(3, 19)] + [(0, n), (n - 1, 1), (n, 0)]
    iv = [(r, 7 * r, 3000 + r, r & 1, -1) for r in range(16)] + [(16, 0, n, 0, -1), (16, n - 33, 33, 1, -1), (17, 0, 1, 1, -1)]
    check(setup, regions, iv, 100)


def test_refusals_leave_the_context_usable(setup):
    eng, chars, regions = setup
    who = "sdf_pool_coverage: "
    for regs, iv, code, text in (
            ([(0, 10), (len(chars) - 5, 10)], [], SDF_ERR_INVALID, "region 1: range outside the resident pool"),
            ([(5, -1)], [], SDF_ERR_INVALID, "region 0: range outside the resident pool"),
            ([(0, 10)], [(0, 0, 1, 0, -1), (0, 5, 6, 0, -1)], SDF_ERR_INVALID, "interval 1: not inside its region"),
            ([(0, 10)], [(0, 5, -1, 0, -1)], SDF_ERR_INVALID, "interval 0: not inside its region"),
            ([(0, 10)], [(0, 0, 1, 2, -1)], SDF_ERR_INVALID, "interval 0: set must be 0 or 1"),
            ([(0, 10)], [(1, 0, 1, 0, -1)], SDF_ERR_INVALID, "interval 0: region out of range"),
            ([(0, 10)], [(0, 0, 1, 0, 1)], SDF_ERR_INVALID, "interval 0: partner out of range"),
            ([(0, 10)], [(0, 0, 1, 0, -2)], SDF_ERR_INVALID, "interval 0: partner out of range")):
        rc, (counts, _, _), err = eng.pool_coverage(regs, iv, 100, check=False)
        assert rc == code and err == who + text and not cover_model.counts_rows(counts).any()
    from sedef_amd.extz2 import COVER_COUNTS_DTYPE, COVER_INTERVAL_DTYPE, POOL_RANGE_DTYPE
    regs, iv, out = np.zeros(1, POOL_RANGE_DTYPE), np.zeros(1, COVER_INTERVAL_DTYPE), np.zeros(1, COVER_COUNTS_DTYPE)
    regs["len"], iv["partner"], iv["len"] = 10, -1, 4
    bad = regs.copy()
    bad["reserved"] = 1
    rc, _, err = eng.pool_coverage(bad, iv, 100, check=False)
    assert rc == SDF_ERR_UNSUPPORTED and err == who + "region 0: reserved must be 0"
    bad = iv.copy()
    bad["reserved"] = 1
    rc, _, err = eng.pool_coverage(regs, bad, 100, check=False)
    assert rc == SDF_ERR_UNSUPPORTED and err == who + "interval 0: reserved must be 0"
    call = eng.lib.sdf_pool_coverage
    assert call(eng.ctx, None, 1, iv.ctypes.data, 1, 100, out.ctypes.data, None, None) == SDF_ERR_INVALID
    assert call(eng.ctx, regs.ctypes.data, 1, None, 1, 100, out.ctypes.data, None, None) == SDF_ERR_INVALID
    assert call(eng.ctx, regs.ctypes.data, 1, iv.ctypes.data, 1, 100, None, None, None) == SDF_ERR_INVALID
    assert call(eng.ctx, None, 0, None, 0, 100, None, None, None) == 0
    assert call(eng.ctx, regs.ctypes.data, 1, iv.ctypes.data, 1, 100, out.ctypes.data, None, None) == 0  # (upper, painted: optional)
    assert int(out["a"][0]) == 4
    check(setup, regions[:3], [(2, 0, 32, 0, -1)], 100)  # the context works on


def test_device_bytes_count_the_bitmaps_and_destroy_frees_them():
    """What the lifecycle tests ask of every buffer of the table (test_gpu_context_lifecycle.py): the process's live bytes rise
    by sdf_device_bytes of the context, to the byte, and are back where they were after sdf_destroy.  The bitmaps are 2 bits a
    base."""
    import sedef_amd
    from sedef_amd.extz2 import live_device_bytes
    gc.collect()
    base = live_device_bytes()
    eng = sedef_amd.Extz2Engine(0)
    n = 1 << 20
    rec = np.frombuffer(b"ACGTacgtN", np.uint8)[np.random.default_rng(5).integers(0, 9, n)]
    cover_cases.upload(eng, [rec])
    before = eng.device_bytes()
    assert live_device_bytes() - base == before
    counts, _, _ = eng.pool_coverage([(0, n)], [(0, 0, n, 0, -1), (0, n // 2, n // 2, 1, -1)], 100)
    assert (cover_model.counts_rows(counts) == cover_model.coverage(rec, [(0, n)], [(0, 0, n, 0, -1), (0, n // 2, n // 2, 1, -1)], 100)[0]).all()
    held = eng.device_bytes()
    assert held - before >= 2 * n // 8  # the bitmaps, and the records beside them
    assert held - before < 2 * n // 8 + (64 << 10)
    assert live_device_bytes() - base == held
    eng.pool_coverage([(0, n // 2)], [(0, 0, 100, 0, -1)], 100)  # a smaller call: nothing grows
    assert eng.device_bytes() == held
    eng.close()
    assert live_device_bytes() == base
