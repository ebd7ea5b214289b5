"""GPU: `sedef stats recall` as a child process (stats_recall.cc over sdf_pair_recall): the device run writes the out.txt and
prints the stdout that the host run (SDF_STATS_RECALL_HOST=1) does, byte for byte -- the text written out in
test_pair_recall_cpu.py -- with and without --ignore-strand."""
import os
import sys

import pytest
import torch  # noqa: F401  (at collection: before the library brings a HIP runtime of its own along)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_pair_recall_cpu as T  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cli():
    from sedef_amd import host
    host.build_host()
    return host.CLI


@pytest.mark.parametrize("extra", [[], ["--ignore-strand"]])
def test_device_run_equals_the_host_run(cli, tmp_path, extra):
    bed, wgac, out_path = T.write_inputs(str(tmp_path))
    host_out = os.path.join(str(tmp_path), "out_host.txt")
    rc, out, err = T.run(cli, ["stats", "recall"] + extra + [bed, wgac, out_path])
    assert rc == 0, err[-2000:]
    rc, out_h, err_h = T.run(cli, ["stats", "recall"] + extra + [bed, wgac, host_out], T.HOST)
    assert rc == 0, err_h[-2000:]
    assert out == out_h and open(out_path).read() == open(host_out).read()
    assert (open(out_path).read(), out) == ((T.OUT_IGNORED, T.STDOUT_IGNORED) if extra else (T.OUT, T.STDOUT))
