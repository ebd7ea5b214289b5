"""`sedef search -t` under SDF_SEARCH_LANES=N as child processes (sedef_amd/csrc/host/search_cmd.cc): several chromosome pairs in
flight, the lines in the loop's order.

Expected stdout: the run with the variable unset, byte for byte, and sdf_search_pair_host per pair through the Python mirror --
no GPU -- as in tests/test_gpu_search_cmd.py, whose FASTA file this is."""
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
    path = str(tmp_path_factory.mktemp("search_lanes_cmd") / "genome.fa")
    G.write_fasta(path, NAMES, RECS, WIDTHS)
    return path


@pytest.fixture(scope="module")
def limit():
    from sedef_amd import host
    return host.limit_table(4096)


def run(cli, args, env):
    base = {k: v for k, v in os.environ.items() if k != "SDF_SEARCH_LANES"}
    return subprocess.run([cli] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120,
                          env=dict(base, SDF_TEST_TRANSLATE_LIMIT=str(GROUP_LIMIT), **env))


@pytest.mark.parametrize("args, qr, rr, reverse, counts", [(["-t"], 0, 1, False, (5, 6)), (["-t", "-r"], 0, 0, True, (4, 4))])
def test_lanes_print_what_the_loop_prints(cli, fasta, limit, args, qr, rr, reverse, counts):
    from sedef_amd import extz2
    assert GROUPS == [["c1", "c2"], ["c3", "c4", "c5"]]
    argv = ["search"] + args + [fasta, str(qr), str(rr)]
    loop, lanes = run(cli, argv, {}), run(cli, argv, {"SDF_SEARCH_LANES": "4"})
    assert loop.returncode == 0 and lanes.returncode == 0, (loop.stderr.decode()[-1000:], lanes.stderr.decode()[-1000:])
    want = G.expected_search(extz2, NAMES, RECS, GROUPS[qr], GROUPS[rr], reverse, limit)
    assert want.count("\n") >= 1
    assert lanes.stdout == loop.stdout == want.encode()
    line = r"Indexes built: %d for %d pairs" % counts
    assert re.search(line + r" \(", loop.stderr.decode()) and re.search(line + r", 4 lanes \(", lanes.stderr.decode())
    # the totals and the three counters are the loop's
    tail = [re.findall(r"(Total:|attempts|Jaccard|interval)\s+=\s+(\d+)", p.stderr.decode()) for p in (loop, lanes)]
    assert len(tail[0]) == 4 and tail[0] == tail[1]


@pytest.mark.parametrize("value", ("0", "17"))
def test_a_lane_count_outside_1_to_16_is_refused_before_a_device_is_opened(cli, fasta, value):
    p = run(cli, ["search", "-t", fasta, "0", "1"], {"SDF_SEARCH_LANES": value, "HIP_VISIBLE_DEVICES": "", "ROCR_VISIBLE_DEVICES": ""})
    assert p.returncode == 1 and p.stdout == b""
    assert ("SDF_SEARCH_LANES=%s: out of range" % value).encode() in p.stderr
