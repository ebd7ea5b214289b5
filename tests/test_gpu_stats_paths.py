"""GPU: the three paths of stats_cols.hip at their edges -- four short alignments in the rows of one wavefront, one
alignment to a wavefront, the segments of a long one -- on the tables of tests/stats_path_cases.py, which
tests/test_stats_paths_cpu.py holds to the edges they name.  Every expected counter is the CPU oracle's
(oracle/stats_oracle.c), for reversed sides on strings reverse-complemented on the host; all sixteen are compared exactly."""
import numpy as np
import pytest
import torch  # noqa: F401  (at collection: before the library brings a HIP runtime of its own along)

import stats_path_cases as spc
from oracle.binding import STATS_FIELDS

pytestmark = pytest.mark.gpu

INVALID = -4  # SDF_ERR_INVALID
_expected = {}


def expect(oracle, case):
    """The oracle's sixteen counters of a case, computed once."""
    a, b, runs = case
    cg = spc.words(runs)
    key = (a, b, cg.tobytes())
    if key not in _expected:
        _expected[key] = oracle.stats_columns(a, b, cg).astype(np.int64)
    return _expected[key]


def as_rows(cols):
    return np.stack([cols[f].astype(np.int64) for f in STATS_FIELDS], axis=1)


@pytest.fixture(scope="module")
def engine():
    """engine(**settings): one context per setting for the module, the tables' pool resident in each."""
    import sedef_amd
    made = {}

    def get(**settings):
        key = tuple(sorted(settings.items()))
        if key not in made:
            made[key] = sedef_amd.Extz2Engine(0, config=settings or None)
            assert made[key].pool_upload(spc.POOL.tobytes()) == len(spc.POOL)
        return made[key]

    yield get
    for eng in made.values():
        eng.close()


def check_batch(eng, oracle, batch, what):
    got = as_rows(eng.stats_columns_batch([(a, b, spc.words(runs)) for a, b, runs in batch]))
    exp = np.stack([expect(oracle, c) for c in batch])
    bad = np.flatnonzero((got != exp).any(axis=1))
    assert len(bad) == 0, (what, len(bad), int(bad[0]), [len(c[2]) for c in batch[bad[0] & ~3:(bad[0] & ~3) + 4]],
                           got[bad[0]].tolist(), exp[bad[0]].tolist())
    return exp


def build(specs):
    from sedef_amd.extz2 import STATS_TASK_DTYPE
    tasks = np.zeros(len(specs), STATS_TASK_DTYPE)
    cig, at = [], 0
    for k, (ao, al, bo, bl, runs, _, _) in enumerate(specs):
        tasks[k] = (ao, bo, al, bl, at, len(runs), 0)
        cig.append(spc.words(runs))
        at += len(runs)
    return tasks, np.concatenate(cig), np.array([s[5] for s in specs], bool), np.array([s[6] for s in specs], bool)


def check_specs(eng, oracle, specs, what):
    tasks, cig, a_rc, b_rc = build(specs)
    got = as_rows(eng.stats_columns_pairs(tasks, cig, a_rc=a_rc, b_rc=b_rc))
    exp = np.stack([expect(oracle, c) for c in spc.as_cases(specs)])
    bad = np.flatnonzero((got != exp).any(axis=1))
    assert len(bad) == 0, (what, len(bad), int(bad[0]), specs[bad[0]][:4], specs[bad[0]][5:], got[bad[0]].tolist(), exp[bad[0]].tolist())
    return exp


# ---- 2. four short alignments in one wavefront ---------------------------------------------------------------------------------
@pytest.mark.parametrize("group_max", spc.GROUP_MAX_SETTINGS, ids=lambda g: "group_max_%s" % ("unset" if g is None else g))
def test_grouped_tables_equal_the_oracle(engine, oracle, group_max):
    """Rows at 0 / 1 / 15 / 16 / 17 / 31 / 32 runs in every position, chunks of 0 .. 33 and 80 units, zero-length runs, sides
    of 0..8 bytes, batch tails and a 33-run alignment in every position of a quad -- counted four to a wavefront, each by
    its own wavefront (0), with one chunk to a row (16) and with four (64): the same records."""
    eng = engine() if group_max is None else engine(SDF_STATS_GROUP_MAX=group_max)
    columns = 0
    for table in spc.GROUP_TABLES:
        for k, batch in enumerate(table.batches):
            exp = check_batch(eng, oracle, batch, (table.name, k))
            assert (exp[:, 15] == 0).all()
            columns += int(exp[:, 14].sum())
    assert columns > 40000  # (the tables are not empty words: that many columns were counted)


def test_strands_in_the_rows_of_a_wavefront(engine, oracle):
    """The four rows of a quad carry the four strand combinations, turned over the row positions: rows of 17..32 runs, sides
    of 0..7 bytes, ranges at the pool's first and last byte."""
    specs = spc.strand_specs()
    exp = check_specs(engine(), oracle, specs, "grouped")
    assert (exp[:, 15] == 0).all() and int(exp[:, 3].sum()) > 500
    check_specs(engine(SDF_STATS_GROUP_MAX=0), oracle, specs, "a wavefront each")
    check_specs(engine(SDF_STATS_GROUP_MAX=16), oracle, specs, "the short quads grouped")
    # the strands matter: without the bits the same tasks count differently
    tasks, cig, _, _ = build(specs)
    plain = as_rows(engine().stats_columns_pairs(tasks, cig))
    assert (plain != exp).any(axis=1).sum() > len(specs) // 3


# ---- 3. a refused alignment beside good ones -------------------------------------------------------------------------------------
def test_refused_alignment_leaves_its_neighbours_alone(engine, oracle):
    """flags == 1 on the refused record and nothing else promised of it; the other rows of its wavefront, and the quad
    before, as the oracle has them; the host form names the first bad alignment."""
    from sedef_amd.extz2 import STATS_COLS_DTYPE, STATS_TASK_DTYPE
    eng = engine()
    for batch, bad, cause, at in spc.refusal_batches():
        tasks = np.zeros(len(batch), STATS_TASK_DTYPE)
        chunks, cigs, off, coff = [], [], 0, 0
        for k, (a, b, runs) in enumerate(batch):
            tasks[k] = (off, off + len(a), len(a), len(b), coff, len(runs), 0)
            off, coff = off + len(a) + len(b), coff + len(runs)
            chunks += [a, b]
            cigs.append(spc.words(runs))
        pool, cig = b"".join(chunks), np.concatenate(cigs)
        out = np.full(len(batch) * 16, -7, np.int32).view(STATS_COLS_DTYPE)
        rc = eng.lib.sdf_stats_columns_batch(eng.ctx, tasks.ctypes.data, len(tasks), pool, len(pool), cig.ctypes.data, len(cig),
                                             out.ctypes.data)
        what = (cause, at, bad)
        assert rc == INVALID, what
        assert eng.lib.sdf_last_error(eng.ctx).decode() == "alignment %d: the CIGAR does not fit its sequences" % bad, what
        got = as_rows(out)
        assert got[bad][15] == 1, what
        for k, case in enumerate(batch):
            if k != bad:
                assert got[k].tolist() == expect(oracle, case).tolist() and got[k][15] == 0, what + (k,)
    # the context serves a good call afterwards
    check_batch(eng, oracle, spc.refusal_batches()[0][0][:4], "after the refusals")


# ---- 4. one alignment to a wavefront, and the segments of a long one ----------------------------------------------------------------
def test_whole_alignments_at_their_chunk_and_round_edges(engine, oracle):
    """33 .. 1024 runs, chunks of 63 .. 193 units, zero-length runs at the seam of the first two chunks."""
    batch = spc.WHOLE_TABLE.batches[0]
    exp = check_batch(engine(), oracle, batch, "default")
    assert (exp[:, 15] == 0).all() and int(exp[:, 14].min()) == 0 and int(exp[:, 14].max()) > 4000
    check_batch(engine(SDF_STATS_GROUP_MAX=0), oracle, batch, "never grouped")
    check_batch(engine(SDF_STATS_ITEMS=1), oracle, batch, "no segment list to speak of")


@pytest.mark.parametrize("n_runs", spc.SEGMENT_COUNTS)
def test_segments_of_a_sole_long_alignment(engine, oracle, n_runs):
    """One long alignment alone in its call, on every strand combination: a list of exactly its segments takes it, a list
    one short -- or of one -- refuses it and its wavefront counts it whole.  Its second segment consumes nothing of a; the
    third of the 1536- and 1537-run ones nothing of b."""
    specs = [s for s in spc.segment_specs() if len(s[4]) == n_runs]
    assert len(specs) == 4
    nseg = spc.segment_count(n_runs)
    exps = []
    for items in (nseg, nseg - 1, 1):
        eng = engine(SDF_STATS_ITEMS=items)
        exps = [check_specs(eng, oracle, [s], ("items", items, s[5:]))[0] for s in specs]
    assert len({e[7:10].tobytes() for e in exps}) >= 3 and all(e[15] == 0 and e[14] > 1500 for e in exps)
    # forward, through the call that brings its own pool; and the four together, with room for all their segments
    check_batch(engine(SDF_STATS_ITEMS=nseg), oracle, spc.as_cases(specs[:1]), "own pool")
    check_specs(engine(), oracle, specs, "together")
