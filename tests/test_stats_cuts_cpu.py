"""f4, host side with the cuts on the device (StatsParams::cuts_device, SDF_STATS_CUTS_DEVICE=1), run without one: the host
builds every piece from the records of sdf_stats_cuts_pairs and the CIGAR alone, and here a CPU stand-in (tests/cuts_model.py)
produces those records from the fetched strings through the hook of sdfh_stats_generate_cuts.

The yardsticks are today's host path (Alignment::trim_front / trim_back are pinned on the reference class,
tests/test_host_pipeline.py) and the column-string model of tests/test_stats_generate.py -- never the kernel."""
import numpy as np
import pytest

import cuts_model
from test_stats_generate import _cols_hook, _handmade, _stage, host, model_table  # noqa: F401  (host: the module's fixture)


def _tables(host, oracle, tmp_path, fa, bed, **kw):
    old, new = str(tmp_path / "host.tsv"), str(tmp_path / "cuts.tsv")
    a = host.stats_generate(fa, bed, old, test_cols=_cols_hook(oracle), **kw)
    calls = []
    hook = cuts_model.hook(calls)
    b = host.stats_generate_cuts(fa, bed, new, test_cols=_cols_hook(oracle), test_cuts=hook, **kw)
    return a, b, open(old).read(), open(new).read(), calls


def test_staged_genome_table_equals_host_path_and_model(host, oracle, tmp_path):
    fa, genome, bed = _stage(host, oracle, tmp_path, seed=21)
    a, b, old, new, calls = _tables(host, oracle, tmp_path, fa, bed)
    assert a == b and a[0] >= 10 and len(calls) == a[1]
    assert new == old
    gen = genome if isinstance(genome, dict) else {"chrT": genome}
    assert new.splitlines()[1:] == model_table(gen, open(bed).read().splitlines())


def test_handmade_assembly_gaps_table_equals_host_path_and_model(host, oracle, tmp_path):
    fa, genome, bed = _handmade(tmp_path, np.random.default_rng(77))
    a, b, old, new, calls = _tables(host, oracle, tmp_path, fa, bed)
    assert a == b and a[1] == 12 and a[2] > a[1]  # alignments were cut
    assert new == old
    assert new.splitlines()[1:] == model_table(genome, open(bed).read().splitlines())
    assert sum(len(c[3]) > 1 for c in calls) >= 4 and any(c[3][0][0] == 0 and len(c[3]) == 1 for c in calls)
    # other filters: pieces that the defaults drop reach the table
    a, b, old, new, _ = _tables(host, oracle, tmp_path, fa, bed, uppercase=10, max_error=0.9)
    assert a == b and new == old
    assert new.splitlines()[1:] == model_table(genome, open(bed).read().splitlines(), uppercase=10, max_error=0.9)


def test_max_ok_gap_takes_todays_path(host, oracle, tmp_path, capfd):
    """--max-ok-gap cuts again through subhit: those trims stay on the host, and so do the first cuts; one line says so."""
    fa, genome, bed = _handmade(tmp_path, np.random.default_rng(77))
    a, b, old, new, calls = _tables(host, oracle, tmp_path, fa, bed, max_ok_gap=0, min_split=200, uppercase=10, max_error=0.9)
    assert a == b and new == old and not calls
    assert new.splitlines()[1:] == model_table(genome, open(bed).read().splitlines(), uppercase=10, max_error=0.9, max_ok_gap=0,
                                               min_split=200)
    err = capfd.readouterr().err
    assert err.count("SDF_STATS_CUTS_DEVICE=1 ignored") == 1


def test_hook_records_describe_the_models_pieces(host, oracle, tmp_path):
    """The records the host consumed in the hand-made run, and the hand-made edge cases of the GPU test, against
    ColAln / _subhit / _split_alignment."""
    fa, genome, bed = _handmade(tmp_path, np.random.default_rng(77))
    calls = []
    hook = cuts_model.hook(calls)
    host.stats_generate_cuts(fa, bed, str(tmp_path / "t.tsv"), test_cols=_cols_hook(oracle), test_cuts=hook)
    assert len(calls) == 12
    for a, b, runs, recs in calls:
        cuts_model.check_against_column_model(a, b, runs, recs)
    cases = cuts_model.handmade(np.random.default_rng(5))
    seen = {}
    for name, a, b, runs in cases:
        recs = cuts_model.records(a, b, runs)
        cuts_model.check_against_column_model(a, b, runs, recs)
        seen[name] = recs
    # what the cases are there for
    assert len(seen["a99"]) == 1 and len(seen["a100"]) == 2 and seen["a101"][1][0] == 251
    assert seen["ab100"][0][:2] == (0, 150) and seen["ba100"][0][:2] == (0, 130)  # a's event comes before b's
    assert len(seen["run to the last column"]) == 1 and seen["run from column 0"] == [(120, 400, 120, 400, seen["run from column 0"][0][4])]
    assert [r[:2] for r in seen["overlapping runs"]] == [(0, 60), (200, 400)]
    assert len(seen["run broken by a gap"]) == 1 and len(seen["gap beside the run"]) == 2
    assert seen["piece starts inside a gap run"][1][:4] == (205, 415, 215, 415)  # (gap_open at the first column: the gap goes)
    assert seen["marker quirk, 5 leading matches"][0] == (0, 25, 0, 0, 0)
    assert seen["marker not met"][0] == (0, 25, 15, 25, 10)
    assert seen["piece of mismatches"][0] == (0, 20, 0, 0, 0)
    assert seen["whole piece scores 0"][0] == (0, 9, 5, 9, 4) and seen["two suffixes of one score"][0] == (0, 13, 0, 13, 8)


def test_existing_entry_points_are_unchanged(host, oracle, tmp_path):
    """sdfh_stats_generate_cuts without the hook and without the setting is sdfh_stats_generate_resident."""
    fa, genome, bed = _handmade(tmp_path, np.random.default_rng(77))
    old, new = str(tmp_path / "a.tsv"), str(tmp_path / "b.tsv")
    a = host.stats_generate(fa, bed, old, test_cols=_cols_hook(oracle))
    b = host.stats_generate_cuts(fa, bed, new, test_cols=_cols_hook(oracle), resident=False, cuts=False)
    assert a == b and open(old).read() == open(new).read()
    with pytest.raises(RuntimeError, match="columns hook"):
        host.stats_generate_cuts(fa, bed, new, test_cuts=cuts_model.hook())


# ---- the array model (cuts_model.records_np) against the column walk, and the seam cases against what they are there for ----
OLD_SCORES = (cuts_model.DEFAULT, (1, -1, -2, -1), (3, 0, 0, -2), (63, -63, -32, -31))  # tests/test_gpu_stats_cuts.py
ALL_SCORES = OLD_SCORES + tuple(s for s in cuts_model.SEAM_SCORES if s not in OLD_SCORES)
LOOP_SPAN = 20000  # the column walk serves as the yardstick up to this span


def _span(runs):
    return sum(n for _, n in runs)


@pytest.fixture(scope="module")
def seams():
    return cuts_model.seam_cases(np.random.default_rng(11))


@pytest.fixture(scope="module")
def small():
    return cuts_model.small_cases(np.random.default_rng(13), 2500)


def _same(a, b, runs, score_sets):
    got = [np.asarray(x) for x in cuts_model.columns(a, b, runs)]
    for x, y in zip(got, cuts_model.columns_np(a, b, runs)):
        assert x.shape == y.shape and (x == y).all()
    for sc in score_sets:
        assert cuts_model.records_np(a, b, runs, sc) == cuts_model.records(a, b, runs, sc), sc


def test_array_model_equals_column_walk_on_the_old_cases():
    for name, a, b, runs in cuts_model.handmade(np.random.default_rng(5)):
        _same(a, b, runs, ALL_SCORES)
    cases = cuts_model.random_cases(np.random.default_rng(9))
    assert len(cases) == 300
    for name, a, b, runs, _, _ in cases:
        _same(a, b, runs, ALL_SCORES)


def test_array_model_equals_column_walk_on_the_seam_cases(seams, small):
    walked = 0
    for family, name, a, b, runs in seams:
        if _span(runs) <= LOOP_SPAN:
            _same(a, b, runs, cuts_model.SEAM_SCORES)
            walked += 1
    assert walked == len(seams)  # (only the 200,000-column case lies above the span)
    for k, (family, name, a, b, runs) in enumerate(small):  # every score set on the first 300, one in turn on the others
        _same(a, b, runs, cuts_model.SEAM_SCORES if k < 300 else cuts_model.SEAM_SCORES[k % 4:k % 4 + 1])


def test_seam_cases_describe_the_column_models_pieces(seams, small):
    for family, name, a, b, runs in seams + small[:200]:
        cuts_model.check_against_column_model(a, b, runs, cuts_model.records_np(a, b, runs))


def _geometry(case, scores=cuts_model.DEFAULT):
    family, name, a, b, runs = case
    kind, na, nb, mt = cuts_model.columns_np(a, b, runs)
    F, G = cuts_model.scores_np(kind, mt, scores)
    return runs, kind, na, nb, mt, cuts_model.events_np(na, nb), cuts_model.records_np(a, b, runs, scores), F, G


def _longest(mask):
    edge = np.diff(np.concatenate(([0], mask.astype(np.int8), [0])))
    return int((np.flatnonzero(edge == -1) - np.flatnonzero(edge == 1)).max(initial=0))


def test_seam_families_do_what_they_are_there_for(seams, small):
    by = {}
    for c in seams:
        assert (c[0], c[1]) not in by
        by[(c[0], c[1])] = c
    fam = lambda f: [c for c in seams if c[0] == f]  # noqa: E731
    assert {c[0] for c in seams} == {"round seam", "long run", "many pieces", "piece edges", "short units", "zero runs", "trim ties", "narrow"}

    # round seam: the event's first column after the run is on either side of column 512 = unit 64 = lane 0 of round 1
    ends = set()
    for c in fam("round seam"):
        runs, kind, na, nb, mt, ev, recs, F, G = _geometry(c)
        if "99 " in c[1]:
            assert not ev and recs == [(0, 1100, 0, 1100, int(mt.sum()))] and _longest(na | nb) == 99
        else:
            assert len(ev) == 1 and len(recs) == 2 and recs[1][0] == ev[0][0] and recs[0][1] == ev[0][2]
            ends.add((c[1][0], ev[0][0], cuts_model.round_of(runs, ev[0][0])[1:]))
            if "starts" in c[1]:
                assert ev[0][2] == int(c[1].split()[-1])
    for side in "ab":
        assert {e for s, e, _ in ends if s == side} >= {504, 511, 512, 513, 519, 520}
        assert {(r, lane) for s, e, (r, lane) in ends if s == side} >= {(0, 63), (1, 0), (1, 1)}

    # long run: N runs over several rounds, and under several chunks of 64 runs
    for side, other in ("ab", "ba"):
        runs, kind, na, nb, mt, ev, recs, F, G = _geometry(by[("long run", "700 on %s, 5000 on %s" % (side, other))])
        assert [e - s for e, _, s in ev] == [700, 5000] and len(recs) == 3
        assert [cuts_model.round_of(runs, e)[1] - cuts_model.round_of(runs, s)[1] for e, _, s in ev] == [1, 10]
    for gap, goes_on in (("D", "a"), ("I", "b")):
        for side in "ab":
            runs, kind, na, nb, mt, ev, recs, F, G = _geometry(by[("long run", "%s 3000 under 200 M10/%s5" % (side, gap))])
            assert len(runs) == 401 and int((na | nb)[300:3300].sum()) == (3000 if side == goes_on else 2000)
            if side == goes_on:
                assert [(e, s) for e, _, s in ev] == [(3300, 300)] and len(recs) == 2
                assert cuts_model.round_of(runs, 3300)[0] - cuts_model.round_of(runs, 300)[0] >= 5
            else:
                assert not ev and len(recs) == 1 and _longest(na | nb) == 10

    # many pieces: more pieces than lanes, written from several chunks and rounds
    for c in fam("many pieces"):
        runs, kind, na, nb, mt, ev, recs, F, G = _geometry(c)
        assert len(ev) == 150 and len(recs) >= 64 and all(100 <= e - s <= 110 for e, _, s in ev)
        assert len({cuts_model.round_of(runs, r[0])[:2] for r in recs}) >= 5 and len({cuts_model.round_of(runs, r[0])[0] for r in recs}) >= 2
        sides = [side for _, side, _ in ev]
        if c[1] == "a":
            assert not any(sides) and len(recs) == 151
        elif c[1] == "alternating":
            assert sides == [0, 1] * 75 and len(recs) == 151
        elif c[1] == "one unit":
            order = {-1: 0, 0: 0, 1: 0}
            for k in range(0, 150, 2):
                (e1, _, s1), (e2, _, s2) = ev[k], ev[k + 1]
                ea, eb = (e1, e2) if ev[k][1] == 0 else (e2, e1)
                assert {ev[k][1], ev[k + 1][1]} == {0, 1} and cuts_model.unit_of(runs, e1) == cuts_model.unit_of(runs, e2)
                assert s2 <= e1  # (a run of 100 that ends inside the unit began before it: the other order cannot be)
                order[(ea > eb) - (ea < eb)] += 1
            assert min(order.values()) >= 10, order
            assert len(recs) == 76
        else:
            for k in range(0, 150, 2):
                (e1, side1, s1), (e2, side2, s2) = ev[k], ev[k + 1]
                assert (side1, side2) == (0, 1) and s1 < s2 < e1 < e2
            assert len(recs) == 76

    # piece edges
    runs, kind, na, nb, mt, ev, recs, F, G = _geometry(by[("piece edges", "every residue")])
    assert {r[0] % 8 for r in recs} == set(range(8)) == {r[1] % 8 for r in recs}
    for edge in (0, 1):
        lanes = {cuts_model.round_of(runs, r[edge])[2] for r in recs if 2000 <= r[edge] < 5000}
        assert lanes >= {63, 0, 1}, lanes
    for name, index in (("an I run", 1), ("a D run", 1), ("the I run at index 63", 63), ("the I run at index 64", 64),
                        ("the D run at index 63", 63), ("the D run at index 64", 64)):
        runs, kind, na, nb, mt, ev, recs, F, G = _geometry(by[("piece edges", "begins inside " + name)])
        j, u, _ = cuts_model.unit_of(runs, recs[1][0])
        assert j == index and runs[j][0] != 0 and recs[1][0] > int(cuts_model.run_starts(runs)[j]) and len(recs) == 2
        assert recs[1][2] > recs[1][0]  # (the trim drops the rest of the gap run)

    # (the idle lanes of the chunk's last round took the gap_open of its last run into the sum the next chunk starts from)
    runs, kind, na, nb, mt, ev, recs, F, G = _geometry(by[("piece edges", "over a chunk that ends with an opening gap")])
    assert runs[63] == (2, 2) and runs[62][0] == 0 and sum((n + 7) // 8 for _, n in runs[:64]) % 64 == 48
    assert recs[1] == (320, 500, 320, 500, 178) and cuts_model.round_of(runs, 320)[0] == 0 and cuts_model.round_of(runs, 499)[0] == 1
    assert F[500] - F[450] == 198 < 16 * 40  # (the tail behind the gap wins by less than the gap_open of the 16 idle lanes)

    # short units
    runs, kind, na, nb, mt, ev, recs, F, G = _geometry(by[("short units", "3000 runs")])
    ops = [op for op, _ in runs]
    assert len(runs) == 3000 and all(1 <= n <= 7 for _, n in runs) and all(x != y for x, y in zip(ops, ops[1:]))
    assert sum((x, y) == (1, 2) for x, y in zip(ops, ops[1:])) >= 20 and sum((x, y) == (2, 1) for x, y in zip(ops, ops[1:])) >= 20
    assert [side for _, side, _ in ev] == [0, 1, 0] and len(recs) == 4

    # zero runs: there, and without a column
    for c in fam("zero runs"):
        runs, kind, na, nb, mt, ev, recs, F, G = _geometry(c)
        zero = [k for k, (_, n) in enumerate(runs) if n == 0]
        assert len(zero) == 1 and len(ev) >= 1
        want = {"at index 63": 63, "at index 64": 64, "first": 0, "last": len(runs) - 1}.get(c[1][4:], 2)
        assert zero == [want], (c[1], zero)
        for sc in cuts_model.SEAM_SCORES:
            assert cuts_model.records_np(c[2], c[3], runs, sc) == cuts_model.records_np(c[2], c[3], [r for r in runs if r[1]], sc)
    # (D 3, D 4 opens once: the ten matches behind the gaps stay; D 3, I 4 opens twice: the twelve matches go)
    assert by[("zero runs", "D 3, M 0, D 4")][4][1:4] == [(1, 3), (0, 0), (1, 4)]
    assert _geometry(by[("zero runs", "D 3, M 0, D 4")])[6][0][:4] == (0, 217, 0, 217)
    assert by[("zero runs", "D 3, M 0, I 4")][4][1:4] == [(1, 3), (0, 0), (2, 4)]
    assert _geometry(by[("zero runs", "D 3, M 0, I 4")])[6][0][:4] == (0, 219, 0, 200)

    # trim ties
    for c in seams:  # with (0, 0, 0, 0) every column of every piece holds the extreme: the column alone decides
        runs, kind, na, nb, mt, ev, recs, F, G = _geometry(c, (0, 0, 0, 0))
        assert not F.any() and not G.any()
        if ev:
            assert all(r[3] == r[1] and r[2] == r[0] or r[2:] == (r[0], r[0], 0) for r in recs)
    runs, kind, na, nb, mt, ev, recs, F, G = _geometry(by[("trim ties", "two maxima, two minima")], (1, -1, 0, 0))
    top = np.flatnonzero(F[1:2001] == F[1:2001].max())
    low = np.flatnonzero(G[:1600] == G[:1600].min())
    assert top.tolist() == [599, 1599] and low.tolist() == [100, 1100] and recs[0] == (0, 2000, 100, 1600, 1000)
    assert cuts_model.round_of(runs, 599)[1] != cuts_model.round_of(runs, 1599)[1] != cuts_model.round_of(runs, 100)[1]
    runs, kind, na, nb, mt, ev, recs, F, G = _geometry(by[("trim ties", "maximum on both sides of a round")], (1, -1, 0, 0))
    top = np.flatnonzero(F[1:701] == F[1:701].max())
    assert top.tolist() == [511, 512, 513, 514] and recs[0] == (0, 700, 0, 515, 512)
    assert cuts_model.round_of(runs, 511) == (0, 0, 63) and cuts_model.round_of(runs, 512) == (0, 1, 0)
    runs, kind, na, nb, mt, ev, recs, F, G = _geometry(by[("trim ties", "deep F")], (63, -63, -32, -31))
    assert F[:4100].min() < -100000 and F[4100] > 0 and recs == [(0, 4100, 2000, 4100, 2100), (4200, 4700, 4200, 4250, 50)]
    for name, gap in (("piece of I columns", 2), ("piece of D columns", 1)):
        runs, kind, na, nb, mt, ev, recs, F, G = _geometry(by[("trim ties", name)], (0, 0, 0, 0))
        assert recs[1][:2] == (170, 250) and (kind[170:250] == gap).all()
        # (all scores equal: trim_front finds column 170, and 170 - 170 = 0 is the number of a-bases of I columns: the marker)
        assert recs[1][2:] == ((170, 170, 0) if gap == 2 else (170, 250, 0))
        assert _geometry(by[("trim ties", name)])[6][2][:4] == ((400, 700, 400, 400) if gap == 2 else (400, 700, 550, 700))

    # narrow
    seen = set()
    for c in fam("narrow"):
        runs, kind, na, nb, mt, ev, recs, F, G = _geometry(c)
        seen.add((len(c[2]), len(c[3]) >= 300) if len(c[2]) < 8 else (len(c[2]) >= 300, len(c[3])))
        assert len(ev) == 1 and len(recs) == 2 and max(len(c[2]), len(c[3])) >= 300
    assert seen == {(0, True), (3, True), (7, True), (True, 0), (True, 3), (True, 7)}

    # the batch: short alignments with and without events
    assert all(130 <= _span(c[4]) <= 300 for c in small)
    pieces = [len(cuts_model.records_np(*c[2:])) for c in small]
    assert pieces.count(1) >= 500 and pieces.count(2) >= 300 and pieces.count(3) >= 30


def test_real_size_case():
    c = cuts_model.real_size_case(np.random.default_rng(12))
    runs, kind, na, nb, mt, ev, recs, F, G = _geometry(c)
    assert len(kind) == 200000 and 380 <= len(runs) <= 450 and all(n for _, n in runs)
    assert [(e - s, side) for e, side, s in ev] == [(50000, 0), (120, 1)] and ev[0][2] == 61000
    assert [r[:2] for r in recs] == [(0, 61000), (111000, ev[1][2]), (ev[1][0], 200000)]
    assert cuts_model.round_of(runs, 111000)[0] - cuts_model.round_of(runs, 61000)[0] >= 1
