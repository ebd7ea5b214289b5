"""bench.py --dump-outputs without a GPU: dump_outputs on made-up results -- what lands in which file, the 64 MB bound,
and a sample that depends on the inputs alone."""
import os

import numpy as np

import bench
from sedef_amd import RESULT_DTYPE


def _results(rng, qlen, tlen):
    """Records with random fields and CIGARs of up to qlen + tlen words, placed in the buffer in a shuffled order."""
    n = len(qlen)
    res = np.zeros(n, RESULT_DTYPE)
    for f in bench.DUMP_FIELDS:
        res[f] = rng.integers(-1000, 1000, n)
    res["n_cigar"] = rng.integers(0, np.minimum(qlen + tlen, 40) + 1)
    order = rng.permutation(n)
    starts = np.cumsum(res["n_cigar"][order]) - res["n_cigar"][order]
    res["cigar_off"][order] = starts
    cigs = rng.integers(0, 1 << 31, int(res["n_cigar"].sum()) + 5).astype(np.uint32)
    return res, cigs


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_dump_holds_every_record_field_and_each_cigar_in_task_order(tmp_path):
    rng = np.random.default_rng(1)
    qlen, tlen = rng.integers(1, 30, 200), rng.integers(1, 30, 200)
    res, cigs = _results(rng, qlen, tlen)
    bench.dump_outputs(str(tmp_path), res, cigs, qlen, tlen)
    got = _load(str(tmp_path))
    assert set(got) == set(bench.DUMP_FIELDS) | {"task", "cigar_task", "cigar"}
    assert all(v.dtype == np.float64 for v in got.values())
    assert np.array_equal(got["task"], np.arange(200)) and np.array_equal(got["cigar_task"], np.arange(200))
    for f in bench.DUMP_FIELDS:
        assert np.array_equal(got[f], res[f].astype(np.float64)), f
    want = np.concatenate([cigs[o:o + c] for o, c in zip(res["cigar_off"], res["n_cigar"])])
    assert np.array_equal(got["cigar"], want.astype(np.float64))


def test_dump_samples_by_the_inputs_alone_within_the_budgets(tmp_path):
    rng = np.random.default_rng(2)
    qlen, tlen = rng.integers(1, 500, 5000), rng.integers(1, 500, 5000)
    res, cigs = _results(rng, qlen, tlen)
    res2, cigs2 = _results(np.random.default_rng(3), qlen, tlen)  # other outputs of the same inputs
    kw = dict(record_bytes=80 * 700, cigar_bytes=200000)
    bench.dump_outputs(str(tmp_path / "a"), res, cigs, qlen, tlen, **kw)
    bench.dump_outputs(str(tmp_path / "b"), res2, cigs2, qlen, tlen, **kw)
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert np.array_equal(a["task"], b["task"]) and np.array_equal(a["cigar_task"], b["cigar_task"])
    tasks, ctasks = a["task"].astype(np.int64), a["cigar_task"].astype(np.int64)
    assert len(tasks) == 700 and np.all(np.diff(tasks) > 0)
    assert 0 < len(ctasks) < 700 and np.all(np.diff(ctasks) > 0) and set(ctasks) <= set(tasks)
    assert 8 * (qlen[ctasks] + tlen[ctasks] + 2).sum() <= 200000
    assert np.array_equal(a["score"], res["score"][tasks].astype(np.float64))
    want = np.concatenate([cigs[res["cigar_off"][k]:res["cigar_off"][k] + res["n_cigar"][k]] for k in ctasks])
    assert np.array_equal(a["cigar"], want.astype(np.float64))


def test_dump_of_a_headline_sized_batch_stays_under_64_mb(tmp_path):
    n = 100000
    qlen, tlen = np.full(n, 1000, np.int32), np.full(n, 1100, np.int32)
    res, cigs = _results(np.random.default_rng(4), qlen, tlen)
    bench.dump_outputs(str(tmp_path), res, cigs, qlen, tlen)
    assert sum(os.path.getsize(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)) <= 64 * 10 ** 6
    assert len(np.load(os.path.join(tmp_path, "task.npy"))) == n
