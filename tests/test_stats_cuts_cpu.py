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
