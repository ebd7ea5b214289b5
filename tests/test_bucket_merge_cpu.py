"""CPU: `align bucket` on records (include/sedef_hip.h: sdf_bucket_merge_host) -- the two models of tests/bucket_model.py against
each other, the `_host` form against them and against host.merge (which the reference pins: tests/test_host_pipeline.py), the
tie claim, the command's files rebuilt from records, and every refusal."""
import gzip
import json
import os

import numpy as np
import pytest

import bucket_model as M
import hostgen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -4, -3


@pytest.fixture(scope="module")
def bk():
    from sedef_amd import bucket
    from sedef_amd.build import build_library
    build_library()
    return bucket


@pytest.fixture(scope="module")
def host():
    from sedef_amd import host as h
    from sedef_amd.build import build_library
    build_library()
    h.build_host()
    return h


def host_form(bk, c, hits=None, **over):
    p = dict(c, **over)
    rc, out = bk.bucket_merge_host(c["hits"] if hits is None else hits, p["chr_group"], p["order"],
                                   bk.bucket_params(p["nbins"], p["extend_ratio"], p["max_extend"], p["merge_dist"]))
    return rc, [tuple(int(x) for x in r) for r in out]


def lines_case(lines):
    """BED lines of one group -> (names, a case with extension stripped)."""
    f = [ln.split("\t") for ln in lines if ln]
    names = sorted({x[0] for x in f} | {x[3] for x in f}, key=lambda s: s.encode())
    ids = {nm: k for k, nm in enumerate(names)}
    hits = [(ids[x[0]], int(x[1]), int(x[2]), ids[x[3]], int(x[4]), int(x[5]), int(x[9] == "-")) for x in f]
    return names, M.case(hits, nbins=1, n_chr=len(names), extend_ratio=0.0)


def merge_cases():
    with gzip.open(os.path.join(ROOT, "tests", "golden", "host_align_kat.json.gz"), "rb") as f:
        out = [c["lines"] for c in json.loads(f.read().decode())["merges"]]
    rng = np.random.default_rng(8)
    return out + [hostgen.merge_case(rng)[0] for _ in range(200)]


def test_the_two_models_agree_on_every_case():
    for name, c in M.cases().items():
        assert M.literal(**c) == M.closed(**c) == M.closed(**dict(c, seed=5)), name
    rng = np.random.default_rng(3)
    for it in range(60):
        c = M.case(M.random_hits(rng, int(rng.integers(1, 200)), n_chr=4, span=int(rng.choice([3000, 30000]))), nbins=int(rng.integers(1, 9)),
                   chr_group=[0, 1, 2, 1], n_groups=3, extend_ratio=float(rng.choice([0, 0.5, 5])), merge_dist=int(rng.choice([0, 250])))
        assert M.literal(**c) == M.closed(**dict(c, seed=it)), it
    for lines in merge_cases():
        c = lines_case(lines)[1]
        assert M.literal(**c) == M.closed(**c)


def test_host_form_equals_the_models_on_every_case(bk):
    for name, c in M.cases().items():
        assert host_form(bk, c) == (0, M.literal(**c)), name
    rng = np.random.default_rng(4)
    for it in range(40):
        c = M.case(M.random_hits(rng, int(rng.integers(1, 300)), n_chr=5, span=20000), nbins=int(rng.integers(1, 9)), chr_group=[0, 1, 2, 1, 0],
                   n_groups=3, extend_ratio=float(rng.choice([0, 0.5, 5])), merge_dist=int(rng.choice([0, 250])))
        assert host_form(bk, c) == (0, M.literal(**c)), it


def test_host_form_equals_host_merge_on_the_golden_cases_and_200_draws(bk, host):
    seen = 0
    for lines in merge_cases():
        names, c = lines_case(lines)
        rc, got = host_form(bk, c)
        assert rc == 0
        want = [(x[0], int(x[1]), int(x[2]), x[3], int(x[4]), int(x[5]), x[9]) for x in
                (ln.split("\t") for ln in host.merge(lines, 250).split("\n") if ln)]
        assert [(names[r[0]], r[1], r[2], names[r[3]], r[4], r[5], "-" if r[6] else "+") for r in got] == want
        seen += len(want)
    assert seen > 2000


def test_hits_that_share_a_sort_key_may_come_in_any_order(bk):
    rng = np.random.default_rng(6)
    shuffled = 0
    for it in range(40):
        base = M.random_hits(rng, 60, n_chr=2, span=4000)
        hits = []
        for h in base:  # ties: the same starts with other ends, twice over
            hits += [h, (h[0], h[1], h[2] + int(rng.integers(0, 900)), h[3], h[4], h[5] + int(rng.integers(0, 900)), h[6]), h]
        c = M.case(hits, nbins=4, n_chr=2)
        want = M.literal(**c)
        assert host_form(bk, c) == (0, want)
        for _ in range(3):
            perm = [hits[k] for k in rng.permutation(len(hits))]
            shuffled += perm != hits
            assert M.literal(**dict(c, hits=perm)) == want and M.closed(**dict(c, hits=perm, seed=it)) == want
            assert host_form(bk, c, hits=perm) == (0, want)
    assert shuffled > 100


def write_genome_index(path, lengths):
    """(the command reads the index alone: names and lengths for the groups)"""
    open(path, "w").write("")
    with open(path + ".fai", "w") as f:
        off = 0
        for name, n in lengths:
            f.write("%s\t%d\t%d\t60\t61\n" % (name, n, off))
            off += n + n // 60 + 10


def search_seeds(rng, names, n, span):
    lines = []
    for h in M.random_hits(rng, n, n_chr=len(names), span=span):
        lines.append("%s\t%d\t%d\t%s\t%d\t%d\t\t\t+\t%s\t%d\t0\t\t;OK" % (names[h[0]], h[1], h[2], names[h[3]], h[4], h[5], "-" if h[6] else "+",
                                                                         max(h[2] - h[1], h[5] - h[4])))
    return lines


def read_dir(d):
    return {n: open(os.path.join(d, n)).read() for n in sorted(os.listdir(d))}


@pytest.mark.parametrize("nbins", [1, 3, 7, 400])
def test_bucket_files_rebuilt_from_records_equal_the_host_path(host, tmp_path, nbins):
    """Three groups (the index alone is read: 100 Mb a group), names whose order is not their number's, more bins than hits at 400."""
    names = ["chr1", "chr10", "chr2", "chrX", "chr21"]
    fa = str(tmp_path / "g.fa")
    write_genome_index(fa, [("chr1", 90 * 10 ** 6), ("chr10", 50 * 10 ** 6), ("chr2", 80 * 10 ** 6), ("chrX", 40 * 10 ** 6), ("chr21", 10 ** 7)])
    groups = host.translation(fa)
    assert len(groups) == 3
    seeds = tmp_path / "seeds"
    seeds.mkdir()
    rng = np.random.default_rng(nbins)
    for part in ("a", "b"):
        open(seeds / (part + ".bed"), "w").write("\n".join(search_seeds(rng, names, 150, 300000)) + "\n")
    want, got = tmp_path / "want", tmp_path / "got"
    want.mkdir(), got.mkdir()
    host.bucket(str(seeds), nbins, str(want), fa)
    assert host.bucket_records(str(seeds), nbins, str(got), fa, form=2) is True
    files = read_dir(want)
    assert len(files) == nbins and read_dir(got) == files
    assert 60 < sum(len(v.splitlines()) for v in files.values()) < 300  # (merged, and fewer than 400)


def test_a_named_seed_keeps_the_host_path(host, tmp_path, capfd):
    fa = str(tmp_path / "g.fa")
    write_genome_index(fa, [("chr1", 50000)])
    bed = tmp_path / "s.bed"
    lines = search_seeds(np.random.default_rng(0), ["chr1"], 5, 9000)
    f = lines[2].split("\t")
    f[6] = "hit7"
    open(bed, "w").write("\n".join(lines[:2] + ["\t".join(f)] + lines[3:]) + "\n")
    out = tmp_path / "out"
    out.mkdir()
    assert host.bucket_records(str(bed), 2, str(out), fa, form=2) is False
    assert os.listdir(out) == []
    assert capfd.readouterr().err.count("SDF_BUCKET_DEVICE=1 ignored") == 1


def test_every_shared_check_is_refused(bk):
    good = M.case([(0, 100, 400, 1, 500, 900, 0), (1, 100, 400, 0, 500, 900, 1)], nbins=2, chr_group=[0, 1], n_groups=2, extend_ratio=5.0)
    assert host_form(bk, good)[0] == 0
    top = 2 ** 31 - 1 - 15000 - 250

    def refused(hits=None, **over):
        return host_form(bk, good, hits=hits, **over)[0]

    assert refused(nbins=0) == INVALID
    assert refused(merge_dist=-1) == INVALID
    assert refused(max_extend=-1) == INVALID
    assert refused(extend_ratio=-1.0) == INVALID and refused(extend_ratio=float("nan")) == INVALID
    assert refused(hits=[(2, 100, 400, 1, 500, 900, 0)]) == INVALID and refused(hits=[(0, 100, 400, -1, 500, 900, 0)]) == INVALID  # ids
    assert refused(chr_group=[0, 2]) == INVALID and refused(chr_group=[-1, 0]) == INVALID                                       # groups
    assert refused(order=[0, 1, 2, 4]) == INVALID
    assert refused(hits=[(0, 401, 400, 1, 500, 900, 0)]) == INVALID and refused(hits=[(0, 100, 400, 1, 901, 900, 0)]) == INVALID  # start > end
    assert refused(hits=[(0, -1, 400, 1, 500, 900, 0)]) == INVALID
    assert refused(hits=[(0, 100, top, 1, 500, 900, 0)], extend_ratio=0.0) == 0                                                  # the last coordinate taken
    assert refused(hits=[(0, 100, top + 1, 1, 500, 900, 0)], extend_ratio=0.0) == INVALID
    assert refused(hits=[(0, 0, 429496730, 1, 0, 5, 0)]) == INVALID and refused(hits=[(0, 0, 429496729, 1, 0, 5, 0)]) == 0      # 5 * len < 2^31
    hits = np.zeros(1, bk.SEED_HIT_DTYPE)
    hits[0] = (0, 100, 400, 1, 500, 900, 2, 0)
    assert refused(hits=hits) == INVALID  # an unknown flag
    hits[0] = (0, 100, 400, 1, 500, 900, 0, 1)
    assert refused(hits=hits) == INVALID  # pad
    p = bk.bucket_params(2)
    assert bk.bucket_merge_host(good["hits"], good["chr_group"], good["order"], p, out_cap=1)[0] == INVALID  # out_cap < n
    assert bk.bucket_merge_host(good["hits"], [0] * ((1 << 19) + 1), [0], p)[0] == INVALID                     # n_chr
    assert bk.bucket_merge_host(good["hits"], [0, 0], np.zeros(4097 * 4097, np.int32), p)[0] == INVALID        # n_groups
    rc, out = bk.bucket_merge_host([], [], [0], p)                                                             # n == 0
    assert rc == 0 and len(out) == 0
