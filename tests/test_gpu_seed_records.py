"""GPU: sdf_seed_records and sdf_seed_records_device equal sdf_seed_records_host record for record (seed_records.hip), and the chain
of `sedef seeds` (sdf_seeds_bucket_merge) equals the two host forms one after the other.

The host form is pinned on the BED text by tests/test_seed_records_cpu.py, on these very tables: eight jobs of which the first is
empty, two in a row in the middle are, and the last is, with a job boundary at hit 64 exactly; n around the wavefront and, at
4,097, over more than one block and past a whole one."""
import os
import sys

import numpy as np
import pytest
import torch  # (at collection: before the library brings a HIP runtime of its own along)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import seeds_model as S  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 3  # records behind out[n] that must stay as they were


@pytest.fixture(scope="module")
def eng():
    import sedef_amd
    e = sedef_amd.Extz2Engine(0)
    yield e
    e.close()


def inputs(n):
    from sedef_amd import seeds
    return seeds.pair_hits(S.table_hits(n)), S.table_first(n), seeds.seed_jobs(S.job_rows(S.NAMES, S.TABLE_JOBS))


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda() if a.nbytes else torch.zeros(8, dtype=torch.uint8, device="cuda")


@pytest.mark.parametrize("n", S.TABLE_SIZES)
def test_both_device_forms_equal_the_host_form(eng, n):
    from sedef_amd import bucket, seeds
    hits, first, jobs = inputs(n)
    rc, want = seeds.seed_records_host(hits, first, jobs)
    assert rc == 0 and len(want) == n
    if n > 64:
        assert {int(f) for f in want["flags"]} == {0, 1} and (want["r_start"] < 0).any()  # (both strands, and flips that wrap)
    launches = eng.lib.sdf_last_launches(eng.ctx)
    got = seeds.seed_records(eng, hits, first, jobs, guard=GUARD)
    assert got[:n].tobytes() == want.tobytes(), [(a, b) for a, b in zip(got.tolist(), want.tolist()) if a != b][:4]
    assert (got[n:].view(np.uint8) == 0xEE).all()
    # the `_device` form on torch tensors, a guard of untouched bytes behind out[n]
    d_hits, d_first, d_jobs = up(hits), up(first), up(jobs)
    d_out = torch.full(((n + GUARD) * 32,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # (the tensors were filled on torch's stream)
    seeds.seed_records_device(eng, d_hits.data_ptr(), n, d_first.data_ptr(), d_jobs.data_ptr(), len(jobs), d_out.data_ptr())
    eng.pool_sync()  # (the context's stream)
    raw = d_out.cpu().numpy()
    dev = raw[:n * 32].view(bucket.SEED_HIT_DTYPE)
    assert dev.tobytes() == want.tobytes(), [(a, b) for a, b in zip(dev.tolist(), want.tolist()) if a != b][:4]
    assert (raw[n * 32:] == 0xEE).all()
    assert eng.lib.sdf_last_launches(eng.ctx) == launches + (2 if n else 0)  # (a launch a call; n == 0: none)


def test_the_device_forms_refuse_what_the_host_form_refuses(eng):
    from sedef_amd import seeds
    hits, first, jobs = inputs(65)
    bad_first, bad_last, bad_jobs = first.copy(), first.copy(), jobs.copy()
    bad_first[3] = 70  # (decreases at the next entry)
    bad_last[-1] = 66  # (first[n_jobs] != n)
    bad_jobs["reserved"][6] = 1
    for args, code in (((hits, bad_first, jobs), -4), ((hits, first, bad_jobs), -3), ((hits, bad_last, jobs), -4), ((hits, None, jobs), -4)):
        assert seeds.seed_records_host(*args)[0] == code
        rc, _ = seeds.seed_records(eng, *args, check=False)
        assert rc == code and eng.lib.sdf_last_error(eng.ctx).decode().startswith("sdf_seed_records: ")
    assert seeds.seed_records(eng, hits, first, jobs, n=(1 << 30) + 1, check=False)[0] == -3
    # what the host can see of the device form: n, n_jobs, the pointers
    assert seeds.seed_records_device(eng, None, (1 << 30) + 1, None, None, 0, None, check=False) == -3
    assert seeds.seed_records_device(eng, None, 5, None, None, 2, None, check=False) == -4
    d = up(hits)
    assert seeds.seed_records_device(eng, d.data_ptr(), 5, d.data_ptr(), d.data_ptr(), 0, d.data_ptr(), check=False) == -4
    assert seeds.seed_records_device(eng, None, 0, None, None, 0, None, check=False) == 0


def test_the_chain_equals_the_two_host_forms(eng):
    """sdf_seeds_bucket_merge on hits the merge takes: the records of sdf_bucket_merge_host on those of sdf_seed_records_host;
    with one flip below 0 among them: dropped, and no records."""
    from sedef_amd import bucket, seeds
    rng = np.random.default_rng(12)
    n = 700
    starts = rng.integers(0, 100000, (n, 2))
    hits = seeds.pair_hits(np.stack([starts[:, 0], starts[:, 0] + rng.integers(700, 3000, n), starts[:, 1], starts[:, 1] + rng.integers(700, 3000, n)], 1))
    first = np.array([0, 0, 200, 200, 200, 450, n, n], np.uint64)
    jobs = seeds.seed_jobs([(0, 0, 4000000, 0), (1, 0, 4000000, 1), (2, 2, 4000000, 0), (3, 1, 4000000, 0), (1, 2, 4000000, 0), (2, 1, 4000000, 1), (3, 3, 4000000, 1)])
    chr_group, order, P = np.array([0, 1, 0, 1], np.int32), bucket.pair_order(2), bucket.bucket_params(3, extend_ratio=0.2, max_extend=300)
    rc, recs = seeds.seed_records_host(hits, first, jobs)
    assert rc == 0
    rc, want = bucket.bucket_merge_host(recs, chr_group, order, P)
    assert rc == 0 and 10 < len(want) < n
    got, dropped = seeds.seeds_bucket_merge(eng, hits, first, jobs, chr_group, order, P)
    assert dropped == 0 and got.tobytes() == want.tobytes()
    short = jobs.copy()
    short["ref_len"][5] = 1000  # (a reverse job whose hits end beyond its reference: their flips are negative)
    got, dropped = seeds.seeds_bucket_merge(eng, hits, first, short, chr_group, order, P)
    assert dropped > 0 and len(got) == 0
