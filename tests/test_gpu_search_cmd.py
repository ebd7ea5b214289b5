"""`sedef search` and `sedef translate` as child processes on a generated FASTA file (sedef_amd/csrc/host/search_cmd.cc).

Expected stdout: sdf_search_pair_host per pair through the Python mirror -- no GPU --, on the same characters and the table
the command computes, pair order and BED text by the models of tests/search_cmd_gen.py.  The seeds were chosen on the CPU so
that every case prints at least one line and the inverted copy is found under -r alone; the test asserts both."""
import os
import re
import subprocess
import sys

import pytest
import torch  # noqa: F401  (at collection: before the library brings a HIP runtime of its own along)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import search_cmd_gen as G  # noqa: E402

pytestmark = pytest.mark.gpu

# five records of 3-12 kb; copies of 1.5-2.5 kb at 3-8 % divergence inside the first record and between records, the one
# into c4 INVERTED; lowercase stretches and an N run; line widths 60 and 70, the last line without a newline
NAMES = ["c1", "c2", "c3", "c4", "c5"]
LENS = [12000, 9000, 7000, 5000, 3000]
COPIES = [(0, 500, 2500, 0, 7000, 0.05, False), (0, 3500, 2000, 1, 1000, 0.04, False), (1, 5000, 1800, 2, 3000, 0.08, False),
          (0, 9800, 1600, 3, 2000, 0.03, True), (2, 500, 1500, 4, 800, 0.06, False)]
RECS = G.records(5, LENS, COPIES, lower=[(0, 2000, 300), (1, 1200, 200), (3, 100, 400)], n_runs=[(2, 6000, 150)])
WIDTHS = [60, 70, 60, 70, 60]
GROUP_LIMIT = 22000  # (test-only, SDF_TEST_TRANSLATE_LIMIT): groups [c1, c2] and [c3, c4, c5]
GROUPS = G.translation_model(list(zip(LENS, NAMES)), GROUP_LIMIT)


@pytest.fixture(scope="module")
def cli():
    from sedef_amd import host
    host.build_host()
    return host.CLI


@pytest.fixture(scope="module")
def fasta(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("search_cmd") / "genome.fa")
    G.write_fasta(path, NAMES, RECS, WIDTHS)
    assert not open(path, "rb").read().endswith(b"\n")
    return path


@pytest.fixture(scope="module")
def limit():
    from sedef_amd import host
    return host.limit_table(4096)


def run(cli, args, env=None):
    p = subprocess.run([cli] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120,
                       env=dict(os.environ, **(env or {})))
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return p.stdout.decode(), p.stderr.decode()


def expected(limit, qr, rr, reverse=False, **kw):
    from sedef_amd import extz2
    text = G.expected_search(extz2, NAMES, RECS, qr, rr, reverse, limit, **kw)
    assert text.count("\n") >= 1
    return text


def indexes_built(err):
    return int(re.search(r"Indexes built: (\d+) for (\d+) pairs", err).group(1)), int(re.search(r"for (\d+) pairs", err).group(1))


def test_a_named_pair(cli, fasta, limit):
    out, err = run(cli, ["search", fasta, "c1", "c2"])
    assert out == expected(limit, ["c1"], ["c2"])
    assert indexes_built(err) == (2, 1) and "READ_SIZE      = 700" in err and "Total:" in err


def test_a_record_against_itself(cli, fasta, limit):
    out, err = run(cli, ["search", fasta, "c1", "c1"])
    assert out == expected(limit, ["c1"], ["c1"])
    assert indexes_built(err) == (1, 1)


def test_the_inverted_copy_is_found_under_r_alone(cli, fasta, limit):
    from sedef_amd import extz2
    assert G.expected_search(extz2, NAMES, RECS, ["c1"], ["c4"], False, limit) == ""
    out, _ = run(cli, ["search", fasta, "c1", "c4"])
    assert out == ""
    out, err = run(cli, ["search", "-r", fasta, "c1", "c4"])
    want = expected(limit, ["c1"], ["c4"], reverse=True)
    assert out == want and all(line.split("\t")[9] == "-" for line in want.splitlines())
    assert indexes_built(err) == (2, 1)
    # the same record on both strands is two indexes, and no same_genome
    out, err = run(cli, ["search", "--reverse", fasta, "c4", "c4"])
    assert out == G.expected_search(extz2, NAMES, RECS, ["c4"], ["c4"], True, limit) and indexes_built(err) == (2, 1)


def test_groups_against_groups(cli, fasta, limit):
    env = {"SDF_TEST_TRANSLATE_LIMIT": str(GROUP_LIMIT)}
    assert GROUPS == [["c1", "c2"], ["c3", "c4", "c5"]]
    out, err = run(cli, ["search", "-t", fasta, "0", "0"], env)
    assert out == expected(limit, GROUPS[0], GROUPS[0])
    assert indexes_built(err) == (2, 4)  # g indexes for g * g pairs
    out, err = run(cli, ["search", "-t", fasta, "0", "1"], env)
    assert out == expected(limit, GROUPS[0], GROUPS[1])
    assert indexes_built(err) == (5, 6)


def test_a_larger_u_loses_a_hit(cli, fasta, limit):
    out, _ = run(cli, ["search", "-u", "600", fasta, "c1", "c1"])
    want = expected(limit, ["c1"], ["c1"], min_uppercase=600)
    assert out == want
    assert set(expected(limit, ["c1"], ["c1"]).splitlines()) - set(want.splitlines())


def test_a_given_limit_table_equal_to_the_computed_one(cli, fasta, limit, tmp_path):
    table = str(tmp_path / "limit.txt")
    with open(table, "w") as f:
        f.write("".join("%d\n" % v for v in limit[1:]))
    out, _ = run(cli, ["search", "--limit-table", table, fasta, "c1", "c2"])
    assert out == expected(limit, ["c1"], ["c2"])
    with open(table, "w") as f:  # a table shorter than the query's minimizers is refused, not read past
        f.write("1\n1\n")
    p = subprocess.run([cli, "search", "--limit-table", table, fasta, "c1", "c2"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 1 and p.stdout == b"" and b"Limit table" in p.stderr


def test_translate_prints_the_models_count(cli, fasta):
    out, err = run(cli, ["translate", fasta], {"SDF_TEST_TRANSLATE_LIMIT": str(GROUP_LIMIT)})
    assert out == "%d\n" % len(GROUPS) and "[Translate] 0 -> c1, c2" in err and "[Translate] 1 -> c3, c4, c5" in err
    out, _ = run(cli, ["translate", fasta])
    assert out == "1\n"
