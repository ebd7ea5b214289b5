"""CPU: `sedef stats diff` as a child process with SDF_STATS_DIFF_HOST=1 -- the command's host layer (stats_diff.cc) over
sdf_pool_coverage_host, no device -- against the lines the model computes (cover_model.stats_diff_lines); the argument errors."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import stats_diff_gen as D  # noqa: E402

HOST = {"SDF_STATS_DIFF_HOST": "1"}


@pytest.fixture(scope="module")
def cli():
    from sedef_amd import host
    host.build_host()
    return host.CLI


def test_host_run_prints_the_models_lines(cli, tmp_path):
    fasta, bed, wgac = D.write_inputs(str(tmp_path))
    rc, out, err = D.run(cli, ["stats", "diff", fasta, bed, wgac], HOST)
    assert rc == 0, err[-2000:]
    assert out == ""
    assert D.report(err) == D.expected()
    # the WGAC record beyond its chromosome was clamped, and the log says so; the chrC record's two sides were dropped
    assert "WGAC: 1 records clamped" in err and "2 sides on chromosomes SEDEF does not cover dropped" in err


def test_argument_errors(cli, tmp_path):
    D.check_argument_errors(cli, str(tmp_path), HOST)


def test_unknown_stats_command_stays(cli, tmp_path):
    fasta, bed, wgac = D.write_inputs(str(tmp_path))
    rc, _, err = D.run(cli, ["stats", "differ", fasta, bed, wgac], HOST)
    assert rc == 1 and "Unknown stats command" in err
