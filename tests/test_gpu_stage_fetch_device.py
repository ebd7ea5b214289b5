"""`sedef align generate` with SDF_STAGE_FETCH_DEVICE=1: on resident chromosomes a super-batch reads its sequences back from
the device pool (one sdf_pool_fetch_ranges call of 2n ranges) instead of cutting them out of the mapped FASTA.  The output is
byte for byte that of the default run, and the log says how many super-batches took the device path -- all of them."""
import os
import re
import subprocess

import pytest

import test_gpu_stage_resident as res
from test_stage_pairs import _write_stage, golden, host  # noqa: F401  (fixtures and the fixture's materialiser)

pytestmark = pytest.mark.gpu

MARKER = re.compile(r"sequence fetch: (\d+) of (\d+) super-batches read their sequences back from the device pool")
FALLBACK = "cuts its sequences out of the FASTA file"


def run_cli(args, **extra):
    from sedef_amd.host import CLI
    env = dict(os.environ, SDF_STAGE_WS_GIB="1")
    for k in ("SDF_DEVICES", "SDF_STAGE_RESIDENT", "SDF_STAGE_FETCH_DEVICE", "SDF_LANES", "SDF_SUPER_BATCH"):
        env.pop(k, None)
    env.update(extra)
    r = subprocess.run([CLI, "align", "generate"] + args, capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def assert_device_fetch_ran(stderr, runs=1):
    """Every super-batch of every bucket took the device path, and none fell back."""
    found = MARKER.findall(stderr)
    assert len(found) == runs, stderr[-2000:]
    for got, of in found:
        assert int(got) == int(of) > 0, stderr[-2000:]
    assert FALLBACK not in stderr and "SDF_STAGE_RESIDENT=1 ignored" not in stderr, stderr[-2000:]


def test_fixture_stages(host, golden, tmp_path):
    for k, fx in enumerate(golden["stages"]):
        d = tmp_path / ("s%d" % k)
        d.mkdir()
        fa, bed = _write_stage(fx, d)
        args = ["-k", str(fx["kmer"]), fa, bed]
        want = "".join(line + "\n" for line in fx["expect"])
        both = run_cli(args, SDF_STAGE_RESIDENT="1", SDF_STAGE_FETCH_DEVICE="1")
        assert both.stdout == want, k
        if fx["kmer"] <= 15:  # (above, the chromosomes do not become resident and the switch has nothing to read)
            assert_device_fetch_ran(both.stderr)
        # the switch alone: no resident genome, the host path, no marker
        alone = run_cli(args, SDF_STAGE_FETCH_DEVICE="1")
        assert alone.stdout == want and not MARKER.search(alone.stderr) and FALLBACK not in alone.stderr, k


def test_four_buckets_on_three_chromosomes(host, tmp_path):
    fa, lens, dups = res.make_genome(tmp_path, seed=31)
    buckets = res.write_buckets(tmp_path, dups, lens, 4, 128, seed=32)
    run_cli(["-k", "11", fa] + buckets, SDF_SUPER_BATCH="16")
    want = res.outputs(buckets)
    assert sum(len(w) for w in want) > 0 and any(b"\t-\t" in w for w in want)
    for env in (dict(SDF_LANES="2", SDF_SUPER_BATCH="16"), dict(SDF_SUPER_BATCH="64")):
        for b in buckets:
            os.remove(b + ".aligned.bed")
        r = run_cli(["-k", "11", fa] + buckets, SDF_STAGE_RESIDENT="1", SDF_STAGE_FETCH_DEVICE="1", **env)
        assert res.outputs(buckets) == want, env
        assert_device_fetch_ran(r.stderr, runs=4)
        assert sum(int(of) for _, of in MARKER.findall(r.stderr)) == 4 * (128 // int(env["SDF_SUPER_BATCH"]))


def test_a_pair_that_is_not_plain_acgtn(host, tmp_path):
    """The pair of tests/test_gpu_stage_resident.py that holds an `R` and a `-`, in all four combinations of the switches."""
    fa, lens, dups = res.make_genome(tmp_path, seed=41, nsd=3, odd=True)
    bed = os.path.join(str(tmp_path), "bucket_0000")
    with open(bed, "w") as f:
        for qn, a, rn, b, rc, L in dups[:2]:
            f.write("%s\t%d\t%d\t%s\t%d\t%d\t\t\t+\t%s\t%d\t0\t\tOK\n" % (qn, a - 100, a + L + 100, rn, b - 100, b + L + 100,
                                                                         "-" if rc else "+", L))
    args = ["-k", "11", fa, bed]
    want = run_cli(args).stdout
    assert len(want) > 0
    assert run_cli(args, SDF_STAGE_RESIDENT="1").stdout == want
    alone = run_cli(args, SDF_STAGE_FETCH_DEVICE="1")
    assert alone.stdout == want and not MARKER.search(alone.stderr)
    both = run_cli(args, SDF_STAGE_RESIDENT="1", SDF_STAGE_FETCH_DEVICE="1")
    assert both.stdout == want
    assert_device_fetch_ran(both.stderr)
