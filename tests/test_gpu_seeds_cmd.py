"""GPU: `sedef seeds` as a child process writes what sedef.sh's seeding phase writes with one process per job
(sedef_amd/csrc/host/seeds_cmd.cc).

The old way, run once per module: the six `sedef search [-r] -t i j` of a three-chromosome genome in two translation groups,
one after the other, into a directory; then `sedef align bucket -n N` on it with SDF_BUCKET_DEVICE unset.  The new way: `sedef
seeds -n N --seeds-dir ...`.  Seed files and bucket files must be byte-identical.  The genome (tests/seeds_model.py) carries
copies on both strands and two within merge_dist of each other; that the old way's own output has hits on both strands and
fewer merged records than seeds is asserted here."""
import os
import re
import subprocess
import sys

import pytest
import torch  # noqa: F401  (at collection: before the library brings a HIP runtime of its own along)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import seeds_model as S  # noqa: E402

pytestmark = pytest.mark.gpu

JOBS = [(0, 0), (1, 0), (1, 1)]  # (query group, reference group), each on both strands: six processes
REFUSED_EXTEND = 2147480000  # --max-extend: no coordinate of the genome is below 2^31 - 1 - max_extend - merge_dist, so the merge takes no record
FALLBACK = "sedef seeds: the records path ignored"


@pytest.fixture(scope="module")
def cli():
    from sedef_amd import host
    host.build_host()
    return host.CLI


@pytest.fixture(scope="module")
def genome(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("seeds_cmd") / "genome.fa")
    S.write_genome(path)
    assert S.genome_groups() == [["s1", "s2"], ["s3"]]
    return path


def env_of(extra):
    base = {k: v for k, v in os.environ.items() if k not in ("SDF_SEARCH_LANES", "SDF_BUCKET_DEVICE")}
    return dict(base, SDF_TEST_TRANSLATE_LIMIT=str(S.GROUP_LIMIT), **extra)


def files_of(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


def bucket_old(cli, seeds_dir, out, genome, nbins, options=()):
    os.makedirs(out)
    p = subprocess.run([cli, "align", "bucket", "-n", str(nbins)] + list(options) + [seeds_dir, out, genome], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=120, env=env_of({}))
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return files_of(out)


@pytest.fixture(scope="module")
def old(cli, genome, tmp_path_factory):
    """The six search processes and their index builds; `align bucket` for N = 1 and 3 on the host path."""
    d = tmp_path_factory.mktemp("seeds_old")
    seeds_dir = str(d / "seeds")
    os.makedirs(seeds_dir)
    builds = 0
    for i, j in JOBS:
        for m, flag in (("n", []), ("y", ["-r"])):
            p = subprocess.run([cli, "search"] + flag + ["-t", genome, str(i), str(j)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120,
                               env=env_of({}))
            assert p.returncode == 0, p.stderr.decode()[-2000:]
            open(os.path.join(seeds_dir, "%d_%d_%s.bed" % (i, j, m)), "wb").write(p.stdout)
            builds += int(re.search(r"Indexes built: (\d+) for", p.stderr.decode()).group(1))
    seeds = files_of(seeds_dir)
    buckets = {n: bucket_old(cli, seeds_dir, str(d / ("buckets%d" % n)), genome, n) for n in (1, 3)}
    # the inputs exercise the merge: hits on both strands, fewer merged records than seeds
    lines = b"".join(seeds.values()).splitlines()
    strands = {ln.split(b"\t")[9] for ln in lines}
    merged = buckets[1]["bucket_0000"].splitlines()
    assert strands == {b"+", b"-"} and 0 < len(merged) < len(lines)
    assert {ln.split(b"\t")[9] for ln in merged} == {b"+", b"-"}
    return dict(seeds_dir=seeds_dir, seeds=seeds, buckets=buckets, builds=builds, n_seeds=len(lines), dir=d)


def seeds_new(genome, out, nbins, seeds_dir=None, options=(), env=None):
    from sedef_amd import seeds
    p = seeds.seeds_command(genome, out, nbins, seeds_dir=seeds_dir, options=options, env=env_of(env or {}), timeout=120)
    assert p.returncode == 0 and p.stdout == b"", p.stderr.decode()[-2000:]
    return files_of(out), p.stderr.decode()


@pytest.mark.parametrize("lanes", (None, 3))
@pytest.mark.parametrize("nbins", (1, 3))
def test_one_process_writes_the_seed_files_and_the_bucket_files(cli, genome, old, tmp_path, nbins, lanes):
    out, sd = str(tmp_path / "buckets"), str(tmp_path / "seeds")
    got, log = seeds_new(genome, out, nbins, seeds_dir=sd, env={} if lanes is None else {"SDF_SEARCH_LANES": str(lanes)})
    assert files_of(sd) == old["seeds"] and sorted(old["seeds"]) == ["%d_%d_%s.bed" % (i, j, m) for i, j in JOBS for m in "ny"]
    assert got == old["buckets"][nbins] and sorted(got) == ["bucket_%04d" % b for b in range(nbins)]
    assert FALLBACK not in log
    # every chromosome uploaded once, one index per strand: six builds, where the six processes built more; one block of totals
    built = re.search(r"Indexes built: (\d+) for (\d+) pairs(, 3 lanes)? \((\d+) chromosomes resident", log)
    assert (int(built.group(1)), int(built.group(2)), int(built.group(4))) == (6, 14, 3) and (built.group(3) is None) == (lanes is None)
    assert 6 < old["builds"] and log.count("Total:") == 1 and "Read total %d alignments" % old["n_seeds"] in log
    assert int(re.search(r"Total:\s+=\s+(\d+)", log).group(1)) == old["n_seeds"]


def test_without_a_seeds_dir_no_seed_file_is_written(genome, old, tmp_path):
    got, log = seeds_new(genome, str(tmp_path / "buckets"), 3)
    assert got == old["buckets"][3] and sorted(os.listdir(tmp_path)) == ["buckets"] and FALLBACK not in log


def test_a_merge_the_records_do_not_take_falls_back_to_the_host_path(cli, genome, old, tmp_path):
    options = ["--max-extend", str(REFUSED_EXTEND)]
    want = bucket_old(cli, old["seeds_dir"], str(tmp_path / "old"), genome, 3, options)
    got, log = seeds_new(genome, str(tmp_path / "new"), 3, options=options)
    assert log.count(FALLBACK) == 1 and got == want and b"".join(want.values())
    assert "Read total %d alignments" % old["n_seeds"] in log


def test_r_and_t_are_refused_before_a_device_is_opened(cli, genome, tmp_path):
    for flag in ("-r", "-t"):
        p = subprocess.run([cli, "seeds", flag, "-n", "1", genome, str(tmp_path / "b")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120,
                           env=env_of({"HIP_VISIBLE_DEVICES": "", "ROCR_VISIBLE_DEVICES": ""}))
        assert p.returncode == 1 and b"-r and -t are not taken" in p.stderr
