"""CPU: sdf_pool_coverage_host (sdf_cover_api.hip) against the definition-level model (cover_model.py) -- the shapes the GPU test
runs (cover_cases.py), every refusal with its code, the legal empties, and both character predicates on every byte value."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cover_cases  # noqa: E402
import cover_model  # noqa: E402

SDF_ERR_UNSUPPORTED, SDF_ERR_INVALID = -3, -4


@pytest.fixture(scope="module")
def ext():
    from sedef_amd import extz2
    extz2.load_library()
    return extz2


@pytest.fixture(scope="module")
def pool():
    records, regions = cover_cases.build_pool()
    return np.concatenate(records).tobytes(), regions


def check(ext, chars, regions, iv, min_upper):
    rc, (counts, upper, painted) = ext.pool_coverage_host(chars, regions, iv, min_upper)
    assert rc == 0
    exp_counts, exp_upper, exp_painted = cover_model.coverage(chars, regions, iv, min_upper)
    assert (cover_model.counts_rows(counts) == exp_counts).all()
    assert (upper == exp_upper).all() and (painted == exp_painted).all()
    return exp_counts, upper, painted


def test_edges_and_whole_regions(ext, pool):
    chars, regions = pool
    exp, _, painted = check(ext, chars, regions, cover_cases.edge_case(regions), 100)
    assert painted.all() and (exp[:, 3] > 0).any() and (exp[:, 4] > 0).any() and (exp[:, 2] > 0).any()
    exp, _, _ = check(ext, chars, regions, cover_cases.whole_case(regions), 100)
    assert [int(x) for x in exp[:, 0] + exp[:, 1]] == [n + 1 for _, n in regions]


def test_partner_thresholds(ext, pool):
    chars, regions = pool
    iv, up, pa = cover_cases.partner_case()
    _, upper, painted = check(ext, chars, regions, iv, 100)
    assert upper.tolist() == up and painted.tolist() == pa
    _, _, painted = check(ext, chars, regions, iv, 99)  # (at 99 every pair is painted)
    assert painted.all()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_intervals(ext, pool, seed):
    chars, regions = pool
    check(ext, chars, regions, cover_cases.random_case(regions, seed), 40)


def test_overlapping_regions_have_bitmaps_of_their_own(ext, pool):
    chars, _ = pool
    regions = [(10, 500), (10, 500), (200, 700)]
    exp, _, _ = check(ext, chars, regions, [(0, 0, 300, 0, -1), (1, 100, 300, 1, -1), (2, 0, 700, 0, -1)], 100)
    assert exp[:, :2].tolist() == [[300, 0], [0, 300], [700, 0]]


def test_every_byte_value(ext):
    """'A' .. 'Z' count as upper (N too); of those every one but N counts as an uppercase base; n, r and bytes >= 128 never do."""
    chars = bytes(range(256))
    iv = [(0, c, 1, 0, -1) for c in range(256)] + [(0, 0, 256, 1, -1)]
    rc, (counts, upper, _) = ext.pool_coverage_host(chars, [(0, 256)], iv, 1)
    assert rc == 0
    assert [c for c in range(256) if upper[c]] == list(range(ord("A"), ord("Z") + 1)) and int(upper[256]) == 26
    assert {f: int(counts[f][0]) for f in counts.dtype.names} == dict(a=256, b=256, both=256, a_only=0, b_only=0, a_only_upper=0, b_only_upper=0)
    for c in range(256):  # set 0 alone on one byte: a_only_upper is that byte's predicate
        rc, (counts, _, _) = ext.pool_coverage_host(chars, [(0, 256)], [(0, c, 1, 0, -1)], 1)
        assert rc == 0 and int(counts["a_only"][0]) == 1
        assert int(counts["a_only_upper"][0]) == int(ord("A") <= c <= ord("Z") and c != ord("N")), c
    check(ext, chars, [(0, 256)], [(0, 0, 256, 1, -1), (0, 3, 200, 0, -1)], 1)
    for c in b"NnRr\x80\xce\xff":
        assert bool(cover_model.is_upper(np.array([c]))[0]) == (c in b"NR")
        assert bool(cover_model.is_upper_base(np.array([c]))[0]) == (c in b"R")


def test_legal_empties(ext, pool):
    chars, regions = pool
    rc, (counts, upper, painted) = ext.pool_coverage_host(chars, regions, [], 100)  # n_iv == 0: all counts zero
    assert rc == 0 and not cover_model.counts_rows(counts).any() and len(upper) == 0
    rc, (counts, _, _) = ext.pool_coverage_host(chars, [], [], 100)  # n_regions == 0
    assert rc == 0 and len(counts) == 0
    exp, upper, painted = check(ext, chars, [(5, 0), (len(chars), 0), (0, 10)], [(0, 0, 0, 0, -1), (1, 0, 0, 1, 0), (2, 10, 0, 1, -1)], 100)
    assert not exp.any() and upper.tolist() == [0, 0, 0] and painted.tolist() == [1, 0, 1]
    rc, _ = ext.pool_coverage_host(b"", [(0, 0)], [(0, 0, 0, 0, -1)], 100)  # an empty pool holds the empty region
    assert rc == 0


REFUSALS = [
    ("region outside the pool", [(0, 10), (995, 10)], [], SDF_ERR_INVALID),
    ("region off < 0", [(-1, 10)], [], SDF_ERR_INVALID),
    ("region len < 0", [(5, -1)], [], SDF_ERR_INVALID),
    ("interval len < 0", [(0, 10)], [(0, 5, -1, 0, -1)], SDF_ERR_INVALID),
    ("interval start < 0", [(0, 10)], [(0, -1, 2, 0, -1)], SDF_ERR_INVALID),
    ("interval beyond its region", [(0, 10)], [(0, 5, 6, 0, -1)], SDF_ERR_INVALID),
    ("interval start beyond its region", [(0, 10)], [(0, 11, 0, 0, -1)], SDF_ERR_INVALID),
    ("set 2", [(0, 10)], [(0, 0, 1, 2, -1)], SDF_ERR_INVALID),
    ("set -1", [(0, 10)], [(0, 0, 1, -1, -1)], SDF_ERR_INVALID),
    ("region index", [(0, 10)], [(1, 0, 1, 0, -1)], SDF_ERR_INVALID),
    ("region index < 0", [(0, 10)], [(-1, 0, 1, 0, -1)], SDF_ERR_INVALID),
    ("partner == n", [(0, 10)], [(0, 0, 1, 0, 1)], SDF_ERR_INVALID),
    ("partner < -1", [(0, 10)], [(0, 0, 1, 0, -2)], SDF_ERR_INVALID),
    ("an interval and no region", [], [(0, 0, 0, 0, -1)], SDF_ERR_INVALID),
]


@pytest.mark.parametrize("what,regions,iv,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(ext, what, regions, iv, code):
    rc, (counts, _, _) = ext.pool_coverage_host(bytes(1000), regions, iv, 100)
    assert rc == code and not cover_model.counts_rows(counts).any()


def test_refusals_reserved_and_null(ext):
    lib = ext.load_library()
    chars = bytes(1000)
    regions = np.zeros(1, ext.POOL_RANGE_DTYPE)
    regions["len"] = 10
    iv = np.zeros(1, ext.COVER_INTERVAL_DTYPE)
    iv["partner"] = -1
    assert ext.pool_coverage_host(chars, regions, iv, 100)[0] == 0
    bad = regions.copy()
    bad["reserved"] = 1
    assert ext.pool_coverage_host(chars, bad, iv, 100)[0] == SDF_ERR_UNSUPPORTED
    bad = iv.copy()
    bad["reserved"] = 4
    assert ext.pool_coverage_host(chars, regions, bad, 100)[0] == SDF_ERR_UNSUPPORTED
    out = np.zeros(1, ext.COVER_COUNTS_DTYPE)
    host = lib.sdf_pool_coverage_host
    assert host(chars, 1000, regions.ctypes.data, 1, iv.ctypes.data, 1, 100, out.ctypes.data, None, None) == 0  # (upper, painted: optional)
    assert host(chars, 1000, None, 1, iv.ctypes.data, 1, 100, out.ctypes.data, None, None) == SDF_ERR_INVALID
    assert host(chars, 1000, regions.ctypes.data, 1, None, 1, 100, out.ctypes.data, None, None) == SDF_ERR_INVALID
    assert host(chars, 1000, regions.ctypes.data, 1, iv.ctypes.data, 1, 100, None, None, None) == SDF_ERR_INVALID
    assert host(None, 1000, regions.ctypes.data, 1, iv.ctypes.data, 1, 100, out.ctypes.data, None, None) == SDF_ERR_INVALID
    assert host(None, 0, None, 0, None, 0, 100, None, None, None) == 0
