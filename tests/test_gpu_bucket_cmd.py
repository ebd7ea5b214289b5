"""GPU: `sedef align bucket` with SDF_BUCKET_DEVICE=1 writes the directory the host path writes, as a child process each; a
seeds file with a named hit keeps the host path and says so once."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bucket_model as M  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = ["chr1", "chr10", "chr2", "chrX", "chr21"]
LENGTHS = [90 * 10 ** 6, 50 * 10 ** 6, 80 * 10 ** 6, 40 * 10 ** 6, 10 ** 7]  # (three groups of at most 100 Mb)
FALLBACK = "SDF_BUCKET_DEVICE=1 ignored"


@pytest.fixture(scope="module")
def cli():
    from sedef_amd import host
    host.build_host()
    return host.CLI


@pytest.fixture(scope="module")
def genome(tmp_path_factory):
    """(the command reads the index alone)"""
    path = str(tmp_path_factory.mktemp("bucket_cmd") / "genome.fa")
    open(path, "w").write("")
    with open(path + ".fai", "w") as f:
        off = 0
        for name, n in zip(NAMES, LENGTHS):
            f.write("%s\t%d\t%d\t60\t61\n" % (name, n, off))
            off += n + n // 60 + 10
    return path


def seeds(rng, n, span=300000):
    return ["%s\t%d\t%d\t%s\t%d\t%d\t\t\t+\t%s\t%d\t0\t\t;OK" % (NAMES[h[0]], h[1], h[2], NAMES[h[3]], h[4], h[5], "-" if h[6] else "+",
                                                                 max(h[2] - h[1], h[5] - h[4]))
            for h in M.random_hits(rng, n, n_chr=len(NAMES), span=span)]


def bucket(cli, bed, out, genome, nbins, device):
    os.makedirs(out)
    p = subprocess.run([cli, "align", "bucket", "-n", str(nbins), bed, out, genome], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120,
                       env=dict(os.environ, SDF_BUCKET_DEVICE="1" if device else "0"))
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return {n: open(os.path.join(out, n)).read() for n in sorted(os.listdir(out))}, p.stderr.decode()


def test_the_device_run_writes_the_host_run_s_directory(cli, genome, tmp_path):
    bed = tmp_path / "seeds"
    bed.mkdir()
    rng = np.random.default_rng(21)
    for part in ("a", "b"):
        open(bed / (part + ".bed"), "w").write("\n".join(seeds(rng, 2000)) + "\n")
    want, log0 = bucket(cli, str(bed), str(tmp_path / "host"), genome, 5, False)
    got, log1 = bucket(cli, str(bed), str(tmp_path / "device"), genome, 5, True)
    assert sorted(want) == ["bucket_%04d" % b for b in range(5)] and got == want
    assert 500 < sum(len(v.splitlines()) for v in want.values()) < 4000
    assert FALLBACK not in log0 and FALLBACK not in log1


def test_a_named_hit_keeps_the_host_path_and_says_so_once(cli, genome, tmp_path):
    lines = seeds(np.random.default_rng(22), 300)
    f = lines[150].split("\t")
    f[6] = "hit150"
    lines[150] = "\t".join(f)
    bed = tmp_path / "seeds.bed"
    open(bed, "w").write("\n".join(lines) + "\n")
    want, _ = bucket(cli, str(bed), str(tmp_path / "host"), genome, 3, False)
    got, log = bucket(cli, str(bed), str(tmp_path / "device"), genome, 3, True)
    assert got == want and log.count(FALLBACK) == 1
