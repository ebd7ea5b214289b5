"""CPU: the tables of tests/stats_path_cases.py reach the edges they are meant to reach, by the kernel's own rule for the
path of a task (stats_path_cases.paths, held to the kernel's constants here), and the oracle takes every case as the GPU
test expects it to: the good ones fit, the bad ones are refused.  Without this the GPU test could pass on inputs that
never enter the path it names, as the fuzz call did: 3 of its 304 quads were grouped."""
import os
import re

import numpy as np
import pytest

import stats_path_cases as spc
from stats_path_cases import GROUP_MAX, LONG, SEG, paths

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _constant(path, name):
    src = open(os.path.join(ROOT, "sedef_amd", "csrc", path)).read()
    m = re.search(r"\b%s\s*=\s*(\d+)\s*[,;]" % name, src)
    assert m, (path, name)
    return int(m.group(1))


def test_constants_equal_the_kernel_sources():
    assert _constant("extz2_geom.h", "STATS_GROUP_MAX") == GROUP_MAX
    assert _constant("stats_cols.hip", "STATS_SEG") == SEG
    assert _constant("stats_cols.hip", "STATS_LONG") == LONG
    # the tables' edges follow the constants: two chunks of sixteen to a grouped row, whole segments in a long alignment
    assert GROUP_MAX == 2 * 16 and LONG == 2 * SEG
    assert max(spc.RUN_COUNTS) == GROUP_MAX and min(spc.WHOLE_COUNTS) == GROUP_MAX + 1 and max(spc.WHOLE_COUNTS) == LONG
    assert spc.SEGMENT_COUNTS == (LONG + 1, 3 * SEG, 3 * SEG + 1)


def test_the_path_rule():
    assert paths([]) == []
    assert paths([32, 0, 1, 32]) == ["group"] * 4
    assert paths([32, 0, 33, 32]) == ["whole"] * 4
    assert paths([1, 1, 1, 1, 1025, 1, 1024, 0, 3]) == ["group"] * 4 + ["segments", "whole", "whole", "whole", "group"]
    assert paths([1, 2, 3, 4, 5], 0) == ["whole"] * 5 and paths([2000, 1], 0) == ["segments", "whole"]
    assert paths([16, 17, 16, 16, 16], 16) == ["whole"] * 4 + ["group"]
    assert paths([64, 64, 65], 64) == ["whole"] * 3 and paths([2000] * 4, 4000) == ["group"] * 4
    # a tail's quad holds the tasks that are there
    assert paths([1, 1, 1, 1, 33]) == ["group"] * 4 + ["whole"]


def test_rev_table_equals_the_host_library():
    from sedef_amd import host
    host.build_host()
    chars = "".join(chr(c) for c in range(1, 128))
    _, rc, _ = host.sequence("t", chars, True)
    tab = spc.rev_table()
    assert rc.encode("latin-1") == tab[np.arange(1, 128)][::-1].tobytes() and (tab[:128] == tab[128:]).all()


@pytest.mark.parametrize("table", spc.GROUP_TABLES + [spc.WHOLE_TABLE], ids=lambda t: t.name)
def test_table_reaches_its_cells(table):
    assert table.want.get(GROUP_MAX)
    for group_max in table.want:
        assert table.missing(group_max) == [], (table.name, group_max)
    for batch in table.batches:
        for a, b, runs in batch:
            assert sum(l for _, l in runs) <= 40000 and len(batch) <= 4000


def test_grouped_tables_hold_their_named_quads_and_material():
    runs, units, zero, lengths, tails, rule, gmax = spc.GROUP_TABLES
    quads = {c[1] for b in runs.batches for c in spc.cells(b) if c[0] == "group_quad"}
    assert {(0, 1, 16, 32), (32, 0, 0, 0), (0, 0, 0, 17), (32, 16, 1, 0), (1, 0, 32, 16)} <= quads and len(quads) >= 33
    # material: mixed case, N / n, bytes outside ASCII and soft-masked stretches in the sequences of the tables
    text = b"".join(a + b for t in spc.GROUP_TABLES for batch in t.batches for a, b, _ in batch)
    assert all(ch in text for ch in b"ACGTacgtNn") and any(ch >= 0x80 for ch in text)
    assert re.search(rb"[acgt]{12}", text) and re.search(rb"[ACGT]{12}", text)
    some_ascii = [a for t in spc.GROUP_TABLES for batch in t.batches for a, b, _ in batch if a and max(a + b) < 0x80]
    assert len(some_ascii) > 50  # (most rows take the packed path; those with a byte >= 0x80 the per-column one)
    # every grouped alignment is a few hundred bases, the sixteen runs of 39 columns apart
    for t in (runs, zero, lengths, tails, rule, gmax):
        assert max(len(a) + len(b) for batch in t.batches for a, b, _ in batch) <= 900
    # the group_max table changes path with the setting, the others' short rows never run whole under the default
    n = [len(c[2]) for c in gmax.batches[0]]
    assert len({tuple(paths(n, g)) for g in (GROUP_MAX, 0, 16, 64)}) == 4


def test_quad_rule_batches():
    """One alignment of 33 runs sends its whole quad to wavefronts of their own; the quads beside it stay grouped."""
    batches = spc.quad_rule_batches()
    assert len(batches) == 4
    for pos, batch in enumerate(batches):
        n = [len(c[2]) for c in batch]
        assert len(n) == 12 and n[4 + pos] == 33 and sum(c == 33 for c in n) == 1 and max(n[:4] + n[8:]) <= GROUP_MAX
        assert paths(n) == ["group"] * 4 + ["whole"] * 4 + ["group"] * 4
        n[4 + pos] = 32
        assert paths(n) == ["group"] * 12


def test_strand_table_reaches_its_cells():
    specs = spc.strand_specs()
    assert sorted(spc.STRAND_WANT - spc.strand_cells(specs), key=repr) == []
    assert set(paths([len(s[4]) for s in specs])) == {"group"}
    P = len(spc.POOL)
    for ao, al, bo, bl, runs, _, _ in specs:
        assert 0 <= ao and ao + al <= P and 0 <= bo and bo + bl <= P and spc.need(runs) == (al, bl)
    assert P % 8 != 0 and (spc.POOL >= 0x80).sum() > 20


def test_segment_table_reaches_its_cells():
    specs = spc.segment_specs()
    P = len(spc.POOL)
    hit = set()
    for case, (ao, al, bo, bl, runs, a_rc, b_rc) in zip(spc.as_cases(specs), specs):
        hit |= spc.cells([case])  # (every one alone in its call: the sole claimant of the segment list)
        assert ao + al == P and bo == 0 and bl <= P and sum(l for _, l in runs) <= 40000
    assert sorted(spc.SEGMENT_WANT - hit, key=repr) == []
    assert len({(s[5], s[6]) for s in specs}) == 4
    assert [spc.segment_count(n) for n in spc.SEGMENT_COUNTS] == [3, 3, 4]
    # zero-length runs at segment seams
    assert any(spc.segment_runs(1537)[k][1] == 0 for k in (SEG - 1, SEG, 2 * SEG - 1, 2 * SEG, 3 * SEG))


def test_oracle_accepts_the_good_and_refuses_the_bad(oracle):
    good = spc.all_good_cases()
    assert len(good) > 500
    for a, b, runs in good:
        assert oracle.stats_columns(a, b, spc.words(runs))[15] == 0, (len(a), len(b), runs)
    batches = spc.refusal_batches()
    seen = set()
    for batch, bad, cause, at in batches:
        n = [len(c[2]) for c in batch]
        path = paths(n)[bad]
        seen.add((cause, at, bad & 3, path))
        flags = [int(oracle.stats_columns(a, b, spc.words(runs))[15]) for a, b, runs in batch]
        assert flags == [int(k == bad) for k in range(len(batch))], (cause, at, bad)
        # the run `at` is the first that does not fit: the alignment cut before it is good
        a, b, runs = batch[bad]
        assert oracle.stats_columns(a, b, spc.words(runs[:at]))[15] == 0
        assert oracle.stats_columns(a, b, spc.words(runs[:at + 1]))[15] == 1
        if cause == "a past its end":
            assert spc.need(runs[:at + 1])[0] == len(a) + 1 and spc.need(runs)[1] <= len(b)
        if cause == "b past its end":
            assert spc.need(runs[:at + 1])[1] == len(b) + 1 and spc.need(runs)[0] <= len(a)
        if cause == "op 3":
            assert runs[at][0] == 3 and sum(op > 2 for op, _ in runs) == 1
        if cause == "run longer than both sequences":
            assert runs[at][1] == max(len(a), len(b)) + 1
    assert {(c, at, pos, "group") for c in spc.CAUSES for at in (5, 20) for pos in range(4)} <= seen
    assert {(c, 20, 1, "whole") for c in spc.CAUSES} <= seen


def test_fuzz_call_in_run_count_order_is_grouped():
    from test_stats_columns import fuzz_cases, fuzz_cases_by_run_count, grouped_quads
    first = fuzz_cases()
    assert grouped_quads(first) == (3, 0) and (len(first) + 3) // 4 == 304  # the call as it was: hardly grouped at all
    second = fuzz_cases_by_run_count()
    grouped, second_chunk = grouped_quads(second)
    print("fuzz call by run count: %d of %d quads grouped, %d of them with a row of 17..32 runs" %
          (grouped, (len(second) + 3) // 4, second_chunk))
    assert grouped >= 100 and second_chunk >= 20
    n = [len(c[2]) for c in second]
    assert n == sorted(n) and len(second) >= len(first)
    # every case of the first call is in the second
    import collections
    key = lambda c: (c[0], c[1], tuple(c[2]))  # noqa: E731
    assert not collections.Counter(map(key, first)) - collections.Counter(map(key, second))
