"""The inputs of the `sedef stats diff` tests (test_stats_diff_cpu.py, test_gpu_stats_diff_cmd.py): a generated FASTA of three
records, a final.bed and a wgac.tab written here, and the lines the command must print, by the model of cover_model.py."""
import os
import subprocess

import cover_model
import search_cmd_gen as G

NAMES = ["chrA", "chrB", "chrC"]
LENS = [3000, 2600, 2200]
# lowercase stretches (chrA's is what leaves one side of a hit with 99 uppercase bases, chrC's what leaves a hit with none), N runs
RECS = G.records(11, LENS, [], lower=[(0, 1000, 300), (0, 150, 50), (0, 450, 80), (1, 900, 150), (2, 100, 400)], n_runs=[(0, 250, 20), (0, 600, 40), (1, 1000, 60)])
RECS[0] = RECS[0][:1200] + b"nnnnnRYRYK" + RECS[0][1210:]  # an n run and IUPAC letters under WGAC's bits
WIDTHS = [60, 70, 60]

STATS_HEADER = "#chr1\tstart1\tend1\tchr2\tstart2\tend2\tname\tscore\tstrand1\tstrand2\tmax_len\taln_len\tcomment"


def bed_line(q, qs, qe, r, rs, re_, q_strand="+", r_strand="+"):
    return "\t".join([q, str(qs), str(qe), r, str(rs), str(re_), "", "0.0", q_strand, r_strand, str(max(qe - qs, re_ - rs)), "0"])


BED = "\n".join([
    STATS_HEADER,
    bed_line("chrA", 100, 700, "chrB", 200, 800),
    bed_line("chrA", 1500, 2100, "chrB", 1500, 2150, "+", "-"),
    bed_line("chrA", 901, 1200, "chrB", 500, 800),            # 99 uppercase bases on the first side: a miss
    bed_line("chrB", 2300, 5000, "chrA", 2500, 2900, "-", "+"),  # the end exceeds the record: clamped to 2600
    bed_line("chrC", 120, 320, "chrA", 50, 300),              # chrC is named by this unpainted hit alone
]) + "\n"


def wgac_line(c1, s1, e1, c2, s2, e2, name, strand="+"):
    f = ["."] * 27
    f[0], f[1], f[2], f[5], f[6], f[7], f[8], f[16], f[26] = c1, str(s1), str(e1), strand, c2, str(s2), str(e2), name, "0.95"
    return "\t".join(f)


WGAC = "\n".join([
    "\t".join("col%d" % i for i in range(27)),      # the header line: dropped
    wgac_line("chrA", 400, 1300, "chrB", 700, 1300, "a1"),
    wgac_line("chrA", 2000, 2900, "chrB", 0, 100, "a1"),          # a name seen before: skipped
    wgac_line("chrA_xy", 0, 3000, "chrB", 0, 2600, "long"),       # a chromosome name of 7 characters: skipped
    wgac_line("chrC", 0, 2000, "chrC", 100, 200, "c1", "-"),      # a chromosome SEDEF does not cover
    wgac_line("chrB", 2400, 9000, "chrA", -50, 150, "e1"),        # beyond the chromosome's end, and below 0
    wgac_line("chrU", 0, 100, "chrU", 200, 300, "u1"),            # a chromosome final.bed never names (nor the FASTA)
]) + "\n"


def expected():
    lines, figures = cover_model.stats_diff_lines(dict(zip(NAMES, RECS)), BED, WGAC)
    assert all(x > 0 for x in figures), figures  # (a run of zeros would pass anything)
    assert lines[0] == "SEDEF reading done (in 3, miss 2)!"
    return lines


def write_inputs(folder):
    fasta = os.path.join(folder, "genome.fa")
    G.write_fasta(fasta, NAMES, RECS, WIDTHS)
    assert not open(fasta, "rb").read().endswith(b"\n")
    bed, wgac = os.path.join(folder, "final.bed"), os.path.join(folder, "wgac.tab")
    with open(bed, "w") as f:
        f.write(BED)
    with open(wgac, "w") as f:
        f.write(WGAC)
    return fasta, bed, wgac


def run(cli, args, env=None):
    """The command as a child process; SDF_STATS_DIFF_HOST as `env` says, whatever the caller's environment holds."""
    e = {k: v for k, v in os.environ.items() if k != "SDF_STATS_DIFF_HOST"}
    e.update(env or {})
    p = subprocess.run([cli] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=e)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


def report(stderr):
    """The lines of the command's stderr from "SEDEF reading done" on, without the build's own bracketed notes."""
    lines = stderr.split("\n")
    at = [i for i, x in enumerate(lines) if x.startswith("SEDEF reading done")]
    assert len(at) == 1, stderr
    return [x for x in lines[at[0]:] if x and not x.startswith("[sedef_amd]")]


def check_argument_errors(cli, folder, env):
    """Too few arguments, a missing file of each kind, a short line in either table: exit code 1 and the reason."""
    fasta, bed, wgac = write_inputs(folder)
    rc, out, err = run(cli, ["stats", "diff", fasta, bed], env)
    assert rc == 1 and out == "" and "Not enough arguments to stats" in err
    rc, _, err = run(cli, ["stats", "diff", fasta], env)
    assert rc == 1 and "Not enough arguments to stats" in err
    rc, _, err = run(cli, ["stats", "diff", os.path.join(folder, "none.fa"), bed, wgac], env)
    assert rc == 1 and "Cannot open file" in err and "none.fa" in err
    rc, _, err = run(cli, ["stats", "diff", fasta, os.path.join(folder, "none.bed"), wgac], env)
    assert rc == 1 and "none.bed does not exist" in err
    rc, _, err = run(cli, ["stats", "diff", fasta, bed, os.path.join(folder, "none.tab")], env)
    assert rc == 1 and "none.tab does not exist" in err
    short_bed = os.path.join(folder, "short.bed")
    with open(short_bed, "w") as f:
        f.write(BED + "chrA\t1\t200\tchrB\t1\t200\t\t0.0\t+\n")
    rc, _, err = run(cli, ["stats", "diff", fasta, short_bed, wgac], env)
    assert rc == 1 and "BED line %d" % (BED.count("\n") + 1) in err and "fewer than 10 fields" in err
    short_wgac = os.path.join(folder, "short.tab")
    with open(short_wgac, "w") as f:
        f.write(WGAC + "\t".join(["chrA", "1", "200"] + ["."] * 23) + "\n")
    rc, _, err = run(cli, ["stats", "diff", fasta, bed, short_wgac], env)
    assert rc == 1 and "WGAC line %d" % (WGAC.count("\n") + 1) in err and "fewer than 27 fields" in err
    unknown = os.path.join(folder, "unknown.bed")
    with open(unknown, "w") as f:
        f.write(bed_line("chrZ", 0, 200, "chrA", 0, 200) + "\n")
    rc, _, err = run(cli, ["stats", "diff", fasta, unknown, wgac], env)
    assert rc == 1 and "Chromosome chrZ does not exist" in err
