"""GPU: stats_cuts.hip where its machinery works -- alignments of several rounds of 64 units and several chunks of 64 runs,
N runs, pieces and trims across those seams, more pieces than lanes, runs of length 0, sides shorter than eight bases, an
alignment of 200,000 columns, and calls of more than 1,024 alignments (sdf_stats_cuts_pairs / sdf_stats_cuts_pairs_device).

No expected value comes from the code under test: the records are those of cuts_model.records_np, the array form of the
model, which tests/test_stats_cuts_cpu.py holds against the column walk (cuts_model.records) and against ColAln / _subhit /
_split_alignment on these very cases, and where every family of cuts_model.seam_cases is checked for what it is there for."""
import os
import sys

import numpy as np
import pytest
import torch  # (at collection: before the library brings a HIP runtime of its own along)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cuts_model  # noqa: E402
from test_gpu_stats_cuts import OVERFLOW, STRANDS, Batch, as_lists, compare  # noqa: E402
from test_gpu_stats_resident import rev_table  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def tab():
    return rev_table()


@pytest.fixture(scope="module")
def eng():
    import sedef_amd
    e = sedef_amd.Extz2Engine(0)
    yield e
    e.close()


def lay(tab, cases, strands):
    """The cases in one pool, each on its strand combination; what the alignment reads there is what the model reads."""
    batch = Batch(tab)
    for (family, name, a, b, runs), (a_rc, b_rc) in zip(cases, strands):
        batch.add_strings(family + ": " + name, a, b, runs, a_rc, b_rc)
    batch.finish()
    for k, c in enumerate(cases):
        assert batch.sides(k) == (c[2], c[3]), c[:2]
    return batch


def firsts(exp):
    return np.concatenate(([0], np.cumsum([len(r) for r in exp]))).astype(np.int64)


def check(batch, first, pieces, exp):
    assert np.array_equal(np.asarray(first, np.int64), firsts(exp))
    compare(batch, as_lists(first, pieces), exp)


def on_device(eng, batch, n, scores, cap, room, stream):
    """sdf_stats_cuts_pairs_device on the first n tasks: (used or None, first, the int32 words of `room` records)."""
    dev = torch.device("cuda", 0)
    d_tasks = torch.from_numpy(batch.tasks[:n].view(np.uint8).copy()).to(dev)
    d_cig = torch.from_numpy(batch.cig.view(np.int32).copy()).to(dev)
    d_first = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
    d_out = torch.full((room * 8,), SENTINEL, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    eng.pool_sync()
    used = eng.stats_cuts_pairs_device(d_tasks.data_ptr(), n, 1, d_cig.data_ptr(), d_first.data_ptr(), d_out.data_ptr(), cap,
                                       scores=scores, stream=stream.cuda_stream if stream is not None else None)
    if stream is not None:
        stream.synchronize()
    return (used if stream is None else None), d_first.cpu().numpy(), d_out.cpu().numpy()


def records_of(words, count):
    from sedef_amd.extz2 import STATS_PIECE_DTYPE
    return words[:8 * count].view(STATS_PIECE_DTYPE)


@pytest.fixture(scope="module")
def seam(tab):
    """Every seam case on the four strand combinations in one pool; the model's records once per score set."""
    cases = cuts_model.seam_cases(np.random.default_rng(11))
    batch = lay(tab, cases * 4, [s for s in STRANDS for _ in cases])
    exp = {sc: [cuts_model.records_np(a, b, runs, sc) for _, _, a, b, runs in cases] * 4 for sc in cuts_model.SEAM_SCORES}
    return batch, cases, exp


@pytest.mark.parametrize("scores", cuts_model.SEAM_SCORES, ids=lambda s: "_".join(str(x) for x in s))
def test_seam_cases_host_form(seam, eng, scores):
    batch, cases, exp = seam
    assert eng.pool_upload(batch.pool.tobytes()) == len(batch.pool)
    first, pieces = eng.stats_cuts_pairs(batch.tasks, batch.cig, scores=scores)
    check(batch, first, pieces, exp[scores])


@pytest.mark.parametrize("scores", cuts_model.SEAM_SCORES, ids=lambda s: "_".join(str(x) for x in s))
def test_seam_cases_device_form_on_the_callers_stream(seam, eng, scores):
    batch, cases, exp = seam
    eng.pool_upload(batch.pool.tobytes())
    need = int(firsts(exp[scores])[-1])
    stream = torch.cuda.Stream(device=torch.device("cuda", 0))
    _, first, out = on_device(eng, batch, len(batch.tasks), scores, need, need + 1, stream)
    assert (out[8 * need:] == SENTINEL).all()
    check(batch, first, records_of(out, need), exp[scores])


def test_no_event_matches_equal_the_columns_call(seam, tab, eng):
    """The whole-alignment counter of the count kernel, over several rounds and chunks, against stats_cols.hip."""
    _, cases, exp = seam
    whole = [c for c, r in zip(cases, exp[cuts_model.DEFAULT]) if len(r) == 1 and r[0][0] == 0]
    assert len(whole) == 12 + 2 and max(len(c[4]) for c in whole) == 401  # (the runs of 99, the two runs that the gaps break)
    batch = lay(tab, whole * 4, [s for s in STRANDS for _ in whole])
    eng.pool_upload(batch.pool.tobytes())
    first, pieces = eng.stats_cuts_pairs(batch.tasks, batch.cig)
    got = as_lists(first, pieces)
    cols = eng.stats_columns_pairs(batch.tasks, batch.cig)
    for k, c in enumerate(whole * 4):
        span = sum(n for _, n in c[4])
        assert got[k] == [(0, span, 0, span, int(cols["matches"][k]))] and int(cols["span"][k]) == span, batch.specs[k][0]
        assert got[k] == cuts_model.records_np(*c[2:])


def test_capacity_around_an_alignment_of_151_pieces(seam, tab, eng):
    """Exact and one short, in both forms; on the device also a capacity inside the long alignment."""
    from sedef_amd.extz2 import STATS_PIECE_DTYPE
    _, cases, _ = seam
    by = {(c[0], c[1]): c for c in cases}
    pick = [by[("round seam", "a100 ends at 512+0")], by[("piece edges", "every residue")], by[("many pieces", "alternating")],
            by[("round seam", "b99 ends at 512+1")], by[("trim ties", "two maxima, two minima")]]
    batch = lay(tab, pick, [STRANDS[k % 4] for k in range(len(pick))])
    exp = [cuts_model.records_np(*c[2:]) for c in pick]
    f = firsts(exp)
    need, n = int(f[-1]), len(pick)
    assert [len(r) for r in exp] == [2, 15, 151, 1, 2]
    eng.pool_upload(batch.pool.tobytes())
    # the host's form
    rc, first, pieces, used = eng.stats_cuts_pairs_raw(batch.tasks, batch.cig, cap=need, pieces=np.zeros(need, STATS_PIECE_DTYPE))
    assert rc == 0 and used == need
    check(batch, first.astype(np.int64), pieces, exp)
    buf = np.zeros(need, STATS_PIECE_DTYPE)
    buf.view(np.int32)[:] = SENTINEL
    rc, first, _, used = eng.stats_cuts_pairs_raw(batch.tasks, batch.cig, cap=need - 1, pieces=buf)
    assert rc == OVERFLOW and used == need and np.array_equal(first.astype(np.int64), f)
    assert (buf.view(np.int32)[8 * (need - 1):] == SENTINEL).all()
    # the device's form on the caller's stream
    stream = torch.cuda.Stream(device=torch.device("cuda", 0))
    for cap in (need, need - 1, int(f[2]) + 70):
        _, first, out = on_device(eng, batch, n, cuts_model.DEFAULT, cap, need + 1, stream)
        assert np.array_equal(first, f)
        assert (out[8 * cap:] == SENTINEL).all()  # nothing at or behind the capacity
        below = int(np.searchsorted(f, cap, side="right")) - 1  # alignments whose pieces all lie below the capacity
        assert below == {need: 5, need - 1: 4}.get(cap, 2)
        got = as_lists(first[:below + 1], records_of(out, int(f[below])))
        assert got == exp[:below]


def test_real_size_alignment(tab, eng):
    """200,000 columns (391 rounds, 7 chunks), a 50,000-column N run: once per strand combination, each with another score set."""
    case = cuts_model.real_size_case(np.random.default_rng(12))
    batch = lay(tab, [case] * 4, STRANDS)
    eng.pool_upload(batch.pool.tobytes())
    for k, scores in enumerate(cuts_model.SEAM_SCORES):
        exp = cuts_model.records_np(*case[2:], scores)
        assert len(exp) == 3 and exp[0][1] == 61000 and exp[1][0] == 111000
        first, pieces = eng.stats_cuts_pairs(batch.tasks[k:k + 1], batch.cig, scores=scores)
        assert as_lists(first, pieces) == [exp], (STRANDS[k], scores)


@pytest.fixture(scope="module")
def small(tab):
    cases = cuts_model.small_cases(np.random.default_rng(13), 2500)
    rng = np.random.default_rng(14)
    batch = lay(tab, cases, [STRANDS[int(s)] for s in rng.integers(0, 4, len(cases))])
    return batch, [cuts_model.records_np(*c[2:]) for c in cases]


@pytest.mark.parametrize("n", (2500, 1023, 1024, 1025, 2049, 41, 42, 43))
def test_batch_seams(small, eng, n):
    """More alignments than the scan kernel's 1,024 threads, and last workgroups of one, two and three alignments."""
    batch, exp = small
    eng.pool_upload(batch.pool.tobytes())
    first, pieces = eng.stats_cuts_pairs(batch.tasks[:n], batch.cig)
    assert len(first) == n + 1
    check(batch, first, pieces, exp[:n])
    if n in (2500, 1025, 43):
        need = int(first[-1])
        _, d_first, out = on_device(eng, batch, n, cuts_model.DEFAULT, need, need + 1, torch.cuda.Stream(device=torch.device("cuda", 0)))
        assert (out[8 * need:] == SENTINEL).all()
        check(batch, d_first, records_of(out, need), exp[:n])
