"""GPU: sdf_pair_recall and sdf_pair_recall_device equal sdf_pair_recall_host and the definition (tests/recall_model.py), record
for record, on every case table of tests/recall_cases.py (pair_recall.hip); the records above the LDS cap; the device form's
status words."""
import os
import sys

import numpy as np
import pytest
import torch  # (at collection: before the library brings a HIP runtime of its own along)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import recall_cases as R  # noqa: E402
import recall_model as M  # noqa: E402

pytestmark = pytest.mark.gpu

TABLES = R.tables()


@pytest.fixture(scope="module")
def eng():
    import sedef_amd
    e = sedef_amd.Extz2Engine(0)
    yield e
    e.close()


def as_tuples(a):
    return [tuple(int(x) for x in r) for r in a.tolist()]


def host_form(gold, found, flags):
    from sedef_amd import recall
    rc, out = recall.pair_recall_host(gold, found, flags)
    assert rc == 0
    return as_tuples(out)


def device_form(eng, gold, found, flags):
    """The `_device` form on torch tensors -> (records, (found dropped, gold dropped))."""
    from sedef_amd import recall
    gold, found = recall.pair_recs(gold), recall.pair_recs(found)

    def up(a):
        return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda() if a.nbytes else torch.zeros(8, dtype=torch.uint8, device="cuda")
    d_gold, d_found = up(gold), up(found)
    d_out = torch.full((len(gold) * 16 + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    d_status = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()  # (the tensors were filled on torch's stream)
    recall.pair_recall_device(eng, d_gold.data_ptr(), len(gold), d_found.data_ptr(), len(found), flags, d_out.data_ptr(), d_status.data_ptr())
    eng.pool_sync()  # (the context's stream)
    raw = d_out.cpu().numpy()
    assert (raw[len(gold) * 16:] == 0xEE).all()  # (nothing behind the last record)
    return as_tuples(raw[:len(gold) * 16].view(recall.RECALL_DTYPE)), tuple(int(x) for x in d_status.cpu().numpy())


def flagged(want):
    """what the device form answers where the host forms answer `want`: a WIDE record keeps its n_hits and its flag, no coverage"""
    return [(r[0], 0, 0, r[3]) if r[3] & M.WIDE else r for r in want]


def check(eng, name):
    from sedef_amd import recall
    gold, found, flags = TABLES[name]
    want = R.expected(name)
    assert host_form(gold, found, flags) == want
    assert as_tuples(recall.pair_recall(eng, gold, found, flags)) == want, name
    dev, status = device_form(eng, gold, found, flags)
    assert status == (0, 0) and dev == flagged(want), name
    return want


@pytest.mark.parametrize("name", [n for n in sorted(TABLES) if not n.startswith("random_")])
def test_both_device_forms_equal_the_host_form_and_the_model(eng, name):
    want = check(eng, name)
    if name == "around_the_cap":  # complete from sdf_pair_recall (above), flagged and without coverage from the device form
        wide = [r for r in want if r[3] & M.WIDE]
        assert len(wide) == 2 and all(r[1] > 0 and r[2] > 0 for r in wide)


def test_two_hundred_random_draws(eng):
    for name in sorted(TABLES):
        if name.startswith("random_"):
            check(eng, name)


def test_two_calls_in_a_row_do_not_see_each_others_index(eng):
    """(the second call has fewer and shorter found records: entries and a longest end left over from the first would show)"""
    from sedef_amd import recall
    g1, f1, _ = TABLES["sort_window_seams"]
    g2, f2, _ = TABLES["unions"]
    assert len(f2) < len(f1) and max(r[2] - r[1] for r in f2) < max(r[2] - r[1] for r in f1)
    for _ in range(2):
        assert as_tuples(recall.pair_recall(eng, g1, f1, 0)) == R.expected("sort_window_seams")
        assert as_tuples(recall.pair_recall(eng, g1[:1], f2, 0)) == M.pair_recall(g1[:1], f2, 0, R.CAP)
        assert as_tuples(recall.pair_recall(eng, g2, f2, 0)) == R.expected("unions")
        assert device_form(eng, g2, f2, 0) == (R.expected("unions"), (0, 0))
        assert as_tuples(recall.pair_recall(eng, g2, [], 0)) == [(0, 0, 0, 0)] * len(g2)


def test_the_device_form_drops_and_counts_what_the_host_forms_refuse(eng):
    from sedef_amd import recall
    gold, found, _ = TABLES["unions"]
    want = R.expected("unions")
    bad = [(0, 1100, 1000, 1, 5100, 5400, 0, 0), (0, -5, 1900, 1, 5100, 5900, 0, 0), (-1, 1100, 1900, 1, 5100, 5900, 0, 0),
           (0, 1100, 1900, 1, 5100, 5900, 0, 7), (0, 1100, 1900, 1, 5100, 5900, 4, 0)]
    assert all(M.bad_record(b) for b in bad)
    rows = [tuple(r) + (0,) for r in found]
    planted = bad[:2] + rows[:3] + bad[2:4] + rows[3:] + bad[4:]
    assert recall.pair_recall(eng, gold, planted, 0, check=False)[0] == M.ERR_INVALID
    dev, status = device_form(eng, gold, planted, 0)
    assert status == (5, 0) and dev == want
    gold_rows = [tuple(g) + (0,) for g in gold]
    dev, status = device_form(eng, gold_rows[:2] + bad[:1] + gold_rows[2:] + bad[3:4], planted, 0)
    assert status == (5, 2)
    assert dev == want[:2] + [(0, 0, 0, recall.BAD)] + want[2:] + [(0, 0, 0, recall.BAD)]


def test_refusals_before_any_launch(eng):
    from sedef_amd import recall
    gold, found, _ = TABLES["unions"]
    launches = eng.last_launches()
    assert recall.pair_recall(eng, gold, found, 2, check=False)[0] == M.ERR_UNSUPPORTED
    assert recall.pair_recall(eng, gold + [(0, 9, 5, 1, 5, 9, 0)], found, 0, check=False)[0] == M.ERR_INVALID
    assert recall.pair_recall_device(eng, 256, 4, 256, 4, 2, 256, 256, check=False) == M.ERR_UNSUPPORTED
    assert recall.pair_recall_device(eng, 256, (1 << 30) + 1, 256, 4, 0, 256, 256, check=False) == M.ERR_UNSUPPORTED
    assert recall.pair_recall_device(eng, 256, 4, 256, (1 << 29) + 1, 0, 256, 256, check=False) == M.ERR_UNSUPPORTED
    assert recall.pair_recall_device(eng, None, 4, 256, 4, 0, 256, 256, check=False) == M.ERR_INVALID
    assert recall.pair_recall_device(eng, 256, 4, 256, 4, 0, 256, None, check=False) == M.ERR_INVALID
    assert eng.last_launches() == launches
