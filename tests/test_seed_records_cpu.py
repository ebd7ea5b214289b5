"""CPU: search hits to seed records (include/sedef_hip.h: sdf_seed_records_host) and the pairs and arguments of `sedef seeds`
(sedef_amd/csrc/host/seeds_cmd.cc).

Expected records: Hit::from_bed of the line search_hit_bed prints for the hit, both through the host library -- what `align
bucket` reads where `sedef search` wrote (tests/test_search_cmd_cpu.py pins the line on the reference).  Expected pairs: the
loops of sedef.sh in Python (tests/seeds_model.py)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import search_cmd_gen as G  # noqa: E402
import seeds_model as S  # noqa: E402
from test_search_cmd_cpu import BED_CASES  # noqa: E402

I31 = S.I31
INVALID, UNSUPPORTED = -4, -3


@pytest.fixture(scope="module")
def host():
    from sedef_amd import host as h
    from sedef_amd.build import build_library
    build_library()
    h.build_host()
    return h


@pytest.fixture(scope="module")
def seeds(host):
    from sedef_amd import seeds as s
    return s


def host_form(seeds, names, hits, first, jobs):
    rc, out = seeds.seed_records_host(hits, first, S.job_rows(names, jobs))
    assert rc == 0
    return [tuple(int(x) for x in r) for r in out]


def test_records_of_the_bed_cases_on_both_strands(host, seeds):
    """One job per (case, strand, reference length): lengths at the hit's end, one beyond, well beyond, and 2^31 - 1."""
    names = sorted({c[0] for c in BED_CASES} | {c[1] for c in BED_CASES})
    hits, jobs = [], []
    for qn, rn, qs, qe, rs, re_ in BED_CASES:
        for reverse in (False, True):
            for ref_len in (re_, re_ + 1, 12345 + re_ if re_ < I31 - 12345 else I31, I31):
                hits.append((qs, qe, rs, re_))
                jobs.append((qn, rn, ref_len, reverse))
    first = np.arange(len(jobs) + 1, dtype=np.uint64)
    want = S.records_by_text(host, seeds, names, hits, first, jobs)
    assert len(want) == len(hits) == 56 and host_form(seeds, names, hits, first, jobs) == want
    assert {w[6] for w in want} == {0, 1} and all(w[7] == 0 for w in want)


def test_flip_edges(host, seeds):
    """ref_len == ref_end: the flipped start is 1; ref_len = 2^31 - 1 with a hit at its end and at its start; a reference shorter than
    the hit's end: the flip wraps below 0, as the BED text has it; ref_len = 0."""
    names = ["q", "r"]
    cases = [((10, 900, 100, 1000), 1000, (1, 901)), ((0, 5, I31 - 700, I31), I31, (1, 701)), ((0, 5, 0, 700), I31, (I31 - 699, -(2 ** 31))),
             ((3, 4, 4000, 5000), 100, (-4899, -3899)), ((3, 4, 1, 2), 0, (-1, 0))]
    hits = [c[0] for c in cases]
    jobs = [("q", "r", c[1], True) for c in cases]
    first = np.arange(len(jobs) + 1, dtype=np.uint64)
    got = host_form(seeds, names, hits, first, jobs)
    assert [(g[4], g[5]) for g in got] == [c[2] for c in cases]
    assert got == S.records_by_text(host, seeds, names, hits, first, jobs)
    assert all(g[:4] == (0, h[0], h[1], 1) and g[6:] == (1, 0) for g, h in zip(got, hits))


def test_records_of_200_draws(host, seeds):
    rng = np.random.default_rng(31)
    for draw in range(200):
        n_jobs = int(rng.integers(1, 7))
        sizes = rng.integers(0, 5, n_jobs) * (rng.random(n_jobs) < 0.7)  # (empty jobs anywhere)
        first = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
        n = int(first[-1])
        top = int(rng.choice([2000, 10 ** 8, I31]))
        hits = np.sort(rng.integers(0, top, (n, 2, 2)), axis=2).reshape(n, 4)
        jobs = [(S.NAMES[int(rng.integers(0, 4))], S.NAMES[int(rng.integers(0, 4))], int(rng.integers(0, top + 1)), bool(rng.integers(0, 2)))
                for _ in range(n_jobs)]
        assert host_form(seeds, S.NAMES, hits, first, jobs) == S.records_by_text(host, seeds, S.NAMES, hits, first, jobs), draw


@pytest.mark.parametrize("n", S.TABLE_SIZES)
def test_the_tables_of_the_device_tests_on_the_host_form(host, seeds, n):
    """(the job tables tests/test_gpu_seed_records.py runs: empty jobs first, in the middle twice, last; a boundary at hit 64)"""
    first, hits = S.table_first(n), S.table_hits(n)
    assert len(first) == len(S.TABLE_JOBS) + 1 and first[0] == first[1] and first[3] == first[4] == first[5] and first[7] == first[8] == n
    got = host_form(seeds, S.NAMES, hits, first, S.TABLE_JOBS)
    step = max(1, n // 150)  # (the text of every hit up to 65, of a sample beyond, the boundaries among it)
    at = sorted(set(range(0, n, step)) | {int(x) + d for x in first for d in (-1, 0) if 0 <= int(x) + d < n})
    want = S.records_by_text(host, seeds, S.NAMES, hits, first, S.TABLE_JOBS)
    assert len(got) == n and [got[t] for t in at] == [want[t] for t in at]


def test_pairs_of_a_three_chromosome_genome_in_two_groups(host, seeds, tmp_path):
    path = str(tmp_path / "genome.fa")
    S.write_genome(path)
    groups = S.genome_groups()
    assert groups == [["s1", "s2"], ["s3"]] and host.translation(path, S.GROUP_LIMIT) == groups
    got = seeds.seeds_pairs(path, S.GROUP_LIMIT)
    assert got == S.pairs_model(groups) and len(got) == 2 * (4 + 2 + 1)
    # the six processes of sedef.sh in its order, each with r outside q; the square of a group holds both orders of a pair
    jobs = []
    for p in got:
        if p[:3] not in jobs:
            jobs.append(p[:3])
    assert jobs == [(0, 0, False), (0, 0, True), (1, 0, False), (1, 0, True), (1, 1, False), (1, 1, True)]
    assert [(p[3], p[4]) for p in got[:4]] == [("s1", "s1"), ("s2", "s1"), ("s1", "s2"), ("s2", "s2")]
    assert [p[5] for p in got[:8]] == [True, False, False, True] + [False] * 4
    assert [(p[3], p[4]) for p in got if p[:3] == (1, 0, True)] == [("s3", "s1"), ("s3", "s2")]
    # one group: the full square on both strands
    assert seeds.seeds_pairs(path) == S.pairs_model([["s1", "s2", "s3"]])


def test_arguments(seeds):
    a = seeds.seeds_args(["-n", "7", "genome.fa", "buckets"])
    assert a == dict(k=12, w=16, u=12, nbins=7, extend_ratio=5.0, max_extend=15000, merge_dist=250, seeds_dir="", pos=["genome.fa", "buckets"])
    a = seeds.seeds_args(["-k", "10", "--bins=3", "--max-extend", "100", "-w", "8", "--merge-dist=9", "--extend-ratio", "0.5", "g.fa", "--seeds-dir", "sd",
                          "-u", "20", "out"])
    assert a == dict(k=10, w=8, u=20, nbins=3, extend_ratio=0.5, max_extend=100, merge_dist=9, seeds_dir="sd", pos=["g.fa", "out"])
    for bad, why in ((["-r", "-n", "1", "g", "b"], "-r and -t"), (["-n", "1", "-t", "g", "b"], "-r and -t"), (["--reverse", "-n", "1", "g", "b"], "-r and -t"),
                     (["g", "b"], "number of bins"), (["-n", "1", "g"], "Not enough arguments"), (["-n", "1", "--frob", "g", "b"], "Unknown option"),
                     (["g", "b", "-n"], "needs a value")):
        with pytest.raises(RuntimeError, match=why):
            seeds.seeds_args(bad)


def test_refusals(seeds):
    hits = S.table_hits(5)
    first = np.array([0, 2, 5], np.uint64)
    jobs = seeds.seed_jobs([(0, 1, 100, 0), (1, 1, 100, 1)])
    call = seeds.seed_records_host
    assert call(hits, first, jobs)[0] == 0
    assert call(hits, first, jobs, n=(1 << 30) + 1)[0] == UNSUPPORTED  # (before anything is read)
    assert call(hits, np.array([0, 3, 2], np.uint64), jobs, n=2)[0] == INVALID  # decreasing
    assert call(hits, np.array([1, 2, 5], np.uint64), jobs)[0] == INVALID  # first[0] != 0
    assert call(hits, np.array([0, 2, 4], np.uint64), jobs)[0] == INVALID  # first[n_jobs] != n
    assert call(hits, first, jobs, n=4)[0] == INVALID
    assert call(hits, np.array([0], np.uint64), jobs[:0])[0] == INVALID  # n > 0 without a job
    for nulls in (dict(hits=None, n=5), dict(first=None), dict(jobs=None), dict(out=False)):
        kw = dict(dict(hits=hits, first=first, jobs=jobs), **nulls)
        assert call(kw.pop("hits"), kw.pop("first"), kw.pop("jobs"), **kw)[0] == INVALID, nulls
    for field, value in (("reserved", 1), ("flags", 2), ("flags", 3)):
        bad = jobs.copy()
        bad[field][1] = value
        assert call(hits, first, bad)[0] == UNSUPPORTED, (field, value)
    # n == 0: SDF_OK, with no array at all and with tables of empty jobs; a bad table is still refused
    assert call(None, None, None)[0] == 0
    assert call(hits[:0], np.zeros(3, np.uint64), jobs)[0] == 0
    assert call(hits[:0], np.array([0, 1, 0], np.uint64), jobs)[0] == INVALID
