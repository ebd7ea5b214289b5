"""GPU: `sedef stats diff` as a child process on a generated FASTA file (stats_diff.cc over sdf_pool_coverage): the device run
prints the lines the model computes (cover_model.stats_diff_lines), byte for byte what the host run (SDF_STATS_DIFF_HOST=1)
prints; the argument errors of the device form."""
import os
import sys

import pytest
import torch  # noqa: F401  (at collection: before the library brings a HIP runtime of its own along)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import stats_diff_gen as D  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cli():
    from sedef_amd import host
    host.build_host()
    return host.CLI


def test_device_run_prints_the_models_lines(cli, tmp_path):
    fasta, bed, wgac = D.write_inputs(str(tmp_path))
    rc, out, err = D.run(cli, ["stats", "diff", fasta, bed, wgac])
    assert rc == 0, err[-2000:]
    assert out == ""
    assert D.report(err) == D.expected()
    rc, out_h, err_h = D.run(cli, ["stats", "diff", fasta, bed, wgac], {"SDF_STATS_DIFF_HOST": "1"})
    assert rc == 0 and out_h == ""
    # the same bytes from the first "reading done" line on: the note on the clamped records and the seven figures included
    assert err_h[err_h.index("SEDEF reading done"):] == err[err.index("SEDEF reading done"):]


def test_argument_errors(cli, tmp_path):
    D.check_argument_errors(cli, str(tmp_path), None)
