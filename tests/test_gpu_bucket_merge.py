"""GPU: sdf_bucket_merge and sdf_bucket_merge_device equal sdf_bucket_merge_host record for record (bucket_merge.hip).

The host form is the reference's sweep on records (tests/test_bucket_merge_cpu.py pins it on host.merge and on the models); the
cases are those of tests/bucket_model.py: runs around the 64-slot step of the sweep, the staircase that needs one pass per
window, a window below the first lower_bound, equal reference ends, self hits, groups, names, merge distances, extension at
its clamps, strands, classes at their edges, bins."""
import os
import sys

import numpy as np
import pytest
import torch  # (at collection: before the library brings a HIP runtime of its own along)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bucket_model as M  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = M.cases()


@pytest.fixture(scope="module")
def eng():
    import sedef_amd
    e = sedef_amd.Extz2Engine(0)
    yield e
    e.close()


def params_of(bk, c):
    return bk.bucket_params(c["nbins"], c["extend_ratio"], c["max_extend"], c["merge_dist"])


def host_form(c):
    from sedef_amd import bucket as bk
    rc, out = bk.bucket_merge_host(c["hits"], c["chr_group"], c["order"], params_of(bk, c))
    assert rc == 0
    return out


def device_form(eng, c, hits=None, out_cap=None):
    """The `_device` form on torch tensors -> (records, dropped)."""
    from sedef_amd import bucket as bk
    hits = bk.seed_hits(c["hits"] if hits is None else hits)
    n = len(hits)
    cap = n if out_cap is None else out_cap

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda() if a.nbytes else torch.zeros(8, dtype=torch.uint8, device="cuda")
    d_hits, d_grp, d_ord = up(hits), up(np.asarray(c["chr_group"], np.int32)), up(np.asarray(c["order"], np.int32))
    d_out = torch.full((max(cap, 1) * 32 + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    d_n = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()  # (the tensors were filled on torch's stream)
    bk.bucket_merge_device(eng, d_hits.data_ptr(), n, d_grp.data_ptr(), len(c["chr_group"]), d_ord.data_ptr(), c["n_groups"], params_of(bk, c),
                           d_out.data_ptr(), cap, d_n.data_ptr())
    eng.pool_sync()  # (the context's stream)
    n_out, dropped = (int(x) for x in d_n.cpu().numpy())
    raw = d_out.cpu().numpy()
    assert 0 <= n_out <= cap and (raw[cap * 32:] == 0xEE).all()  # (nothing behind the capacity)
    return raw[:n_out * 32].view(bk.BUCKET_HIT_DTYPE).copy(), dropped


def check(eng, c):
    from sedef_amd import bucket as bk
    want = host_form(c)
    got = bk.bucket_merge(eng, c["hits"], c["chr_group"], c["order"], params_of(bk, c))
    assert got.tobytes() == want.tobytes(), [(a, b) for a, b in zip(got.tolist(), want.tolist()) if a != b][:4]
    dev, dropped = device_form(eng, c)
    assert dropped == 0 and dev.tobytes() == want.tobytes(), [(a, b) for a, b in zip(dev.tolist(), want.tolist()) if a != b][:4]
    return want


@pytest.mark.parametrize("name", sorted(CASES))
def test_both_device_forms_equal_the_host_form(eng, name):
    want = check(eng, CASES[name])
    if name.startswith("run_"):
        assert len(want) == int(name[4:]) + 1  # (every hit of the run survives its sweep)
    if name.startswith("chain_"):
        assert len(want) == 1
    if name == "staircase":
        assert len(want) == len(CASES[name]["hits"]) - 5
    if name == "classes":
        assert len(set(int(b) for b in want["bucket"])) == 3 and len(want) == len(CASES[name]["hits"])


def test_twenty_thousand_random_hits_in_six_chromosomes_and_three_groups(eng):
    rng = np.random.default_rng(11)
    c = M.case(M.random_hits(rng, 20000, n_chr=6, span=400000), nbins=7, chr_group=[0, 1, 2, 1, 0, 2], n_groups=3, extend_ratio=5.0)
    want = check(eng, c)
    assert 1000 < len(want) < 19000


def test_a_run_of_a_thousand_that_collapses_into_few(eng):
    """(every hit of a long run absorbs: passes repeat, slots die, the owner lane of a slot changes with its place)"""
    rng = np.random.default_rng(12)
    blocks = rng.integers(0, 40, 1000)  # forty places in the reference, 400 apart: the hits of a place end up as one
    hits = [(0, 1000 + 7 * i, 1400 + 7 * i, 1, 1000 * int(b), 1000 * int(b) + 600, 0) for i, b in enumerate(blocks)]
    want = check(eng, M.case(hits, nbins=5))
    assert 1 <= len(want) <= 400


def test_the_device_form_drops_and_counts_what_the_host_forms_refuse(eng):
    from sedef_amd import bucket as bk
    c = M.case([(0, 100, 400, 1, 500, 900, 0), (1, 5000, 5400, 0, 6000, 6900, 1), (0, 9000, 9400, 1, 9500, 9900, 0)], nbins=2)
    bad = bk.seed_hits(c["hits"] + [(0, 100, 400, 7, 500, 900, 0), (0, 401, 400, 1, 500, 900, 0), (0, 100, 400, 1, 500, 2 ** 31 - 1, 0)])
    bad = bad[[3, 0, 4, 1, 5, 2]]
    assert bk.bucket_merge(eng, bad, c["chr_group"], c["order"], params_of(bk, c), check=False)[0] == -4
    dev, dropped = device_form(eng, c, hits=bad)
    assert dropped == 3 and dev.tobytes() == host_form(c).tobytes()
    # a table entry out of range drops the records that meet it, and nothing is read outside the tables
    dev, dropped = device_form(eng, dict(c, chr_group=[0, 5]))
    assert dropped == 3 and len(dev) == 0


def test_refusals_of_the_scalars_before_any_launch(eng):
    from sedef_amd import bucket as bk
    c = CASES["two_groups"]
    launches = eng.last_launches()
    for over in (dict(nbins=0), dict(merge_dist=-1), dict(max_extend=-1), dict(extend_ratio=-2.0)):
        assert bk.bucket_merge(eng, c["hits"], c["chr_group"], c["order"], params_of(bk, dict(c, **over)), check=False)[0] == -4
    assert bk.bucket_merge(eng, c["hits"], c["chr_group"], c["order"], params_of(bk, c), out_cap=3, check=False)[0] == -4
    assert bk.bucket_merge_device(eng, 256, 4, 256, 3, 256, 2, params_of(bk, c), 256, 3, 256, check=False) == -4   # out_cap < n
    assert bk.bucket_merge_device(eng, 256, 4, 256, 3, 256, 4097, params_of(bk, c), 256, 4, 256, check=False) == -4  # n_groups
    assert bk.bucket_merge_device(eng, 256, (1 << 30) + 1, 256, 3, 256, 2, params_of(bk, c), 256, 1 << 31, 256, check=False) == -3
    assert eng.last_launches() == launches
