"""CPU: sdf_pair_recall_host against the definition (tests/recall_model.py) on every case table, its refusals, and
`sedef stats recall` under SDF_STATS_RECALL_HOST=1 -- the command's host layer (stats_recall.cc) over that form, no device --
against text written out here."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import recall_cases as R  # noqa: E402
import recall_model as M  # noqa: E402

TABLES = R.tables()
URL = "http://humanparalogy.gs.washington.edu/build37/"


def host_form(gold, found, flags):
    from sedef_amd import recall
    rc, out = recall.pair_recall_host(gold, found, flags)
    return rc, [tuple(int(x) for x in r) for r in out.tolist()]


def test_the_mirror_carries_the_headers_constants():
    from sedef_amd import recall
    assert (recall.CAP, recall.WIDE, recall.IGNORE_STRAND) == (R.CAP, M.WIDE, M.IGNORE_STRAND)
    assert recall.PAIR_REC_DTYPE.itemsize == 32 and recall.RECALL_DTYPE.itemsize == 16


@pytest.mark.parametrize("name", [n for n in sorted(TABLES) if not n.startswith("random_")])
def test_host_form_equals_the_model(name):
    gold, found, flags = TABLES[name]
    rc, got = host_form(gold, found, flags)
    assert rc == 0 and got == R.expected(name)


def test_host_form_equals_the_model_on_two_hundred_random_draws():
    names = [n for n in sorted(TABLES) if n.startswith("random_")]
    assert len(names) == 200
    for name in names:
        gold, found, flags = TABLES[name]
        assert len(gold) <= 300 and len(found) <= 2000
        rc, got = host_form(gold, found, flags)
        assert rc == 0 and got == R.expected(name), name


BAD = {"start_behind_end_1": (0, 11, 10, 1, 5, 9, 0), "start_behind_end_2": (0, 5, 9, 1, 11, 10, 0), "negative_start_1": (0, -1, 10, 1, 5, 9, 0),
       "negative_start_2": (0, 5, 9, 1, -1, 10, 0), "negative_chr_1": (-1, 5, 9, 1, 5, 9, 0), "negative_chr_2": (0, 5, 9, -1, 5, 9, 0),
       "reserved": (0, 5, 9, 1, 5, 9, 0, 1), "flag_bit_2": (0, 5, 9, 1, 5, 9, 4)}


@pytest.mark.parametrize("what", sorted(BAD))
def test_host_form_refuses_a_bad_record_in_either_set(what):
    good = [R.G + (0,), (0, 1400, 1600, 1, 5400, 5600, 0, 0)]
    bad = BAD[what] + (0,) * (8 - len(BAD[what]))
    assert M.bad_record(bad) and not any(M.bad_record(g) for g in good)
    assert host_form(good + [bad], good, 0)[0] == M.ERR_INVALID
    assert host_form(good, [bad] + good, 0)[0] == M.ERR_INVALID
    assert host_form([], [bad], 0)[0] == M.ERR_INVALID  # (checked before n_gold == 0 answers nothing)
    assert host_form(good, good, 0)[0] == 0


def test_host_form_refuses_unknown_call_flags_and_null_pointers():
    from sedef_amd import recall
    assert host_form([R.G], [R.G], 2)[0] == M.ERR_UNSUPPORTED
    L = recall._lib()
    out = np.zeros(1, recall.RECALL_DTYPE)
    g = recall.pair_recs([R.G])
    assert L.sdf_pair_recall_host(None, 1, g.ctypes.data, 1, 0, out.ctypes.data) == M.ERR_INVALID
    assert L.sdf_pair_recall_host(g.ctypes.data, 1, None, 1, 0, out.ctypes.data) == M.ERR_INVALID
    assert L.sdf_pair_recall_host(g.ctypes.data, 1, g.ctypes.data, 1, 0, None) == M.ERR_INVALID
    assert L.sdf_pair_recall_host(g.ctypes.data, 1, None, 0, 0, out.ctypes.data) == 0


# ---- the command -------------------------------------------------------------------------------------------------------------

def bed(c1, s1, e1, c2, s2, e2, st1="+", st2="+"):
    return "\t".join([c1, str(s1), str(e1), c2, str(s2), str(e2), "", "0.0", st1, st2, "x", "y"])


def wgac(c1, s1, e1, strand, c2, s2, e2, name):
    f = [c1, str(s1), str(e1), "n", "0", strand, c2, str(s2), str(e2)] + ["."] * 7 + [name] + ["."] * 12
    assert len(f) == 29 and f[16] == name
    return "\t".join(f)


BED = "\n".join([
    "#chr1\tstart1\tend1\tchr2\tstart2\tend2",
    bed("chr1", 1000, 2000, "chr2", 5000, 6000),              # both: covers it whole, as listed
    bed("chr2", 15000, 15500, "chr1", 11000, 11500),          # second_row: hits the name's second row, crosswise
    bed("chr1", 21000, 21400, "chr3", 25000, 25790),          # tie_a: 40% and 79%
    bed("chr1", 31000, 31400, "chr3", 35000, 35790),          # tie_b: the same
    bed("chr1", 41000, 41795, "chr3", 45000, 46000),          # rounds_up: 79.5% rounds to 80: full
    bed("chr1", 51000, 52000, "chr2", 55000, 56000, "+", "+"),  # stranded: WGAC lists it as '_': a strand mismatch on end 2
    bed("chr1", 61000, 61100, "chr2", 65000, 65100),          # low: 10% and 10%
    bed("chr1", 1500, 2500, "chr2", 5900, 7000),              # both again: nested in the union, beyond the sides
]) + "\n"
WGAC = "\n".join([
    "chrom\tchromStart\tchromEnd\tname\tscore\tstrand\totherChrom\totherStart\totherEnd",
    wgac("chr1", 1000, 2000, "+", "chr2", 5000, 6000, "both"),
    wgac("chr2", 5000, 6000, "+", "chr1", 1000, 2000, "both"),            # the other orientation under the same name
    wgac("chr1", 71000, 72000, "+", "chr2", 75000, 76000, "second_row"),  # no hit on this row
    wgac("chr1", 11000, 11500, "+", "chr2", 15000, 15500, "second_row"),  # full through this one
    wgac("chr1", 21000, 22000, "+", "chr3", 25000, 26000, "tie_b"),
    wgac("chr1", 31000, 32000, "+", "chr3", 35000, 36000, "tie_a"),
    wgac("chr1", 41000, 42000, "+", "chr3", 45000, 46000, "rounds_up"),
    wgac("chr1", 51000, 52000, "_", "chr2", 55000, 56000, "stranded"),
    wgac("chr1", 61000, 62000, "+", "chr2", 65000, 66000, "low"),
    wgac("chr1_gl000191_random", 10, 20, "+", "chr2", 30, 40, "underscore"),
    wgac("chr1", 81000, 81000, "+", "chr2", 85000, 86000, "empty_side"),
    wgac("chr3", 1234567, 2234567, "+", "chr3", 91000, 92000, "nothing"),
    wgac("chr3", 91000, 92000, "+", "chr3", 1234567, 2234567, "nothing"),
]) + "\n"
OUT = ("MISS\tchr3\t91000\t92000\tchr3\t1234567\t2234567\t+\tlen1=1,000\tlen2=1,000,000\t" + URL + "nothing\n"
       "MISS\tchr1\t51000\t52000\tchr2\t55000\t56000\t_\tlen1=1,000\tlen2=1,000\t" + URL + "stranded\n"
       "PART\t10.00\t10.00\t" + URL + "low\n"
       "PART\t40.00\t79.00\t" + URL + "tie_a\n"
       "PART\t40.00\t79.00\t" + URL + "tie_b\n")
STDOUT = ("WGAC:          8 (13 lines)\n"
          "Missed:        2 hits (25.0%)\n"
          "Partial:       3 hits (37.5%)\n"
          "Full:          3 hits (37.5%)\n")
OUT_IGNORED = OUT.replace("MISS\tchr1\t51000\t52000\tchr2\t55000\t56000\t_\tlen1=1,000\tlen2=1,000\t" + URL + "stranded\n", "")
STDOUT_IGNORED = ("WGAC:          8 (13 lines)\n"
                  "Missed:        1 hits (12.5%)\n"
                  "Partial:       3 hits (37.5%)\n"
                  "Full:          4 hits (50.0%)\n")


def write_inputs(folder):
    paths = [os.path.join(folder, n) for n in ("final.bed", "wgac.tab", "out.txt")]
    with open(paths[0], "w") as f:
        f.write(BED)
    with open(paths[1], "w") as f:
        f.write(WGAC)
    return paths


def run(cli, args, env=None):
    """The command as a child process; the two settings as `env` says, whatever the caller's environment holds."""
    e = {k: v for k, v in os.environ.items() if k not in ("SDF_STATS_RECALL_HOST", "SDF_STATS_RECALL_IGNORE_STRAND")}
    e.update(env or {})
    p = subprocess.run([cli] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=e)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


HOST = {"SDF_STATS_RECALL_HOST": "1"}


@pytest.fixture(scope="module")
def cli():
    from sedef_amd import host
    host.build_host()
    return host.CLI


def test_the_written_text_is_what_the_model_computes():
    assert M.stats_recall_text(BED, WGAC) == (OUT, STDOUT, 1)
    assert M.stats_recall_text(BED, WGAC, ignore_strand=True) == (OUT_IGNORED, STDOUT_IGNORED, 1)


def test_command_on_the_host_form_prints_the_written_text(cli, tmp_path):
    bed_p, wgac_p, out_p = write_inputs(str(tmp_path))
    rc, out, err = run(cli, ["stats", "recall", bed_p, wgac_p, out_p], HOST)
    assert rc == 0, err[-2000:]
    assert out == STDOUT and open(out_p).read() == OUT
    assert "1 rows with an empty side skipped" in err


def test_ignore_strand_finds_the_row_the_strand_mismatch_misses(cli, tmp_path):
    bed_p, wgac_p, out_p = write_inputs(str(tmp_path))
    for args, env in ((["stats", "recall", "--ignore-strand", bed_p, wgac_p, out_p], HOST),
                      (["stats", "recall", bed_p, wgac_p, "--ignore-strand", out_p], HOST),
                      (["stats", "recall", bed_p, wgac_p, out_p], dict(HOST, SDF_STATS_RECALL_IGNORE_STRAND="1"))):
        rc, out, err = run(cli, args, env)
        assert rc == 0, err[-2000:]
        assert out == STDOUT_IGNORED and open(out_p).read() == OUT_IGNORED


def test_the_library_entry_gives_the_same(tmp_path):
    from sedef_amd import host
    host.build_host()
    bed_p, wgac_p, out_p = write_inputs(str(tmp_path))
    assert host.stats_recall(bed_p, wgac_p, out_p, host=True) == STDOUT and open(out_p).read() == OUT
    assert host.stats_recall(bed_p, wgac_p, out_p, host=True, ignore_strand=True) == STDOUT_IGNORED and open(out_p).read() == OUT_IGNORED


def test_argument_errors(cli, tmp_path):
    bed_p, wgac_p, out_p = write_inputs(str(tmp_path))
    rc, out, err = run(cli, ["stats", "recall", bed_p, wgac_p], HOST)
    assert rc == 1 and out == "" and "Not enough arguments to stats" in err
    rc, _, err = run(cli, ["stats", "recall", str(tmp_path / "none.bed"), wgac_p, out_p], HOST)
    assert rc == 1 and "none.bed does not exist" in err
    rc, _, err = run(cli, ["stats", "recall", bed_p, str(tmp_path / "none.tab"), out_p], HOST)
    assert rc == 1 and "none.tab does not exist" in err
    rc, _, err = run(cli, ["stats", "recall", bed_p, wgac_p, str(tmp_path / "no" / "such" / "out.txt")], HOST)
    assert rc == 1 and "Cannot write" in err
    short_bed, short_wgac, flipped = (str(tmp_path / n) for n in ("short.bed", "short.tab", "flipped.tab"))
    with open(short_bed, "w") as f:
        f.write(BED + "chr1\t1\t200\tchr2\t1\t200\t\t0.0\t+\n")
    rc, _, err = run(cli, ["stats", "recall", short_bed, wgac_p, out_p], HOST)
    assert rc == 1 and "BED line %d" % (BED.count("\n") + 1) in err and "fewer than 10 fields" in err
    with open(short_wgac, "w") as f:
        f.write(WGAC + "\t".join(["chr1", "1", "200"] + ["."] * 13) + "\n")
    rc, _, err = run(cli, ["stats", "recall", bed_p, short_wgac, out_p], HOST)
    assert rc == 1 and "WGAC line %d" % (WGAC.count("\n") + 1) in err and "fewer than 17 fields" in err
    with open(flipped, "w") as f:
        f.write(WGAC + wgac("chr1", 300, 200, "+", "chr2", 1, 200, "flipped") + "\n")
    rc, _, err = run(cli, ["stats", "recall", bed_p, flipped, out_p], HOST)
    assert rc == 1 and "WGAC line %d" % (WGAC.count("\n") + 1) in err and "behind its end" in err


def test_the_host_form_alone_under_the_address_and_undefined_sanitizers(tmp_path):
    """tests/pair_recall_main.cc: a program of its own around sdf_pair_recall_host, against the definition written out in C++ --
    the lists beyond the cap and the refusals on exact-size arrays included --, its host side built with
    -fsanitize=address,undefined and run here, on the CPU."""
    import shutil
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    src, exe = os.path.join(ROOT, "sedef_amd", "csrc"), str(tmp_path / "pair_recall")
    subprocess.check_call([hipcc, "-std=c++17", "-O1", "-g", "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=address,undefined", "-I", src,
                           os.path.join(src, "pair_recall.hip"), os.path.join(src, "sdf_recall_api.hip"), "-x", "hip",
                           os.path.join(ROOT, "tests", "pair_recall_main.cc"), "-o", exe], stderr=subprocess.DEVNULL)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0 and p.stdout == b"pair recall ok\n" and b"Sanitizer" not in p.stderr and b"runtime error" not in p.stderr, \
        p.stderr.decode()[-2000:]
