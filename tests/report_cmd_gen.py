"""The inputs of the `sedef report` test (tests/test_gpu_report_cmd.py): a generated FASTA of three records that hold copies of
one another, and three overlapping *.aligned.bed files of `align generate` lines (an empty name column, a CIGAR of one run) that
share lines, so that the same alignment leaves several buckets."""
import os

import numpy as np

import search_cmd_gen as G

NAMES = ["chrA", "chr10", "chr2"]
LENS = [9000, 8000, 7000]
WIDTHS = [60, 70, 60]
# (source record, source start, length, target record, target start, reverse strand)
# (1,000 bases and more each: `stats generate` drops shorter pieces; no target range touches a source range)
COPIES = [(0, 200, 1200, 1, 300, False), (0, 2000, 1100, 2, 100, False), (1, 2000, 1300, 2, 2000, True), (0, 4000, 1000, 0, 6500, False),
          (2, 4000, 1050, 1, 4500, False), (1, 6000, 1150, 0, 7700, True)]
KEYS = "-k1,1V -k9,9r -k10,10r -k4,4V -k2,2n -k3,3n -k5,5n -k6,6n"


def genome():
    recs = [bytearray(r) for r in G.records(23, LENS, [])]
    rng = np.random.default_rng(5)
    for src, s0, n, dst, d0, inverted in COPIES:
        piece = bytearray(recs[src][s0:s0 + n])
        for at in rng.choice(n, n // 25, replace=False):  # substitutions alone: the alignment is one run of n columns
            piece[at] = b"ACGT"[(b"ACGT".index(piece[at]) + 1 + int(rng.integers(0, 3))) % 4]
        recs[dst][d0:d0 + n] = G.rev_comp(bytes(piece)) if inverted else bytes(piece)
    return [bytes(r) for r in recs]


def aligned_line(src, s0, n, dst, d0, inverted, comment="m=4.0;g=0.0"):
    return "%s\t%d\t%d\t%s\t%d\t%d\t\t4.0\t+\t%s\t%d\t%d\t%dM\t%s" % (NAMES[src], s0, s0 + n, NAMES[dst], d0, d0 + n, "-" if inverted else "+",
                                                                     n, n, n, comment)


def bucket_files():
    """name -> text.  Every line stands in two files at least; two lines share all eight keys and differ in the comment."""
    lines = [aligned_line(*c) for c in COPIES] + [aligned_line(*COPIES[0], comment="m=4.0;g=0.1")]
    files = {"bucket_0000.aligned.bed": lines[0:4] + lines[6:7], "bucket_0001.aligned.bed": lines[2:7], "bucket_0002.aligned.bed": lines[4:] + lines[0:3]}
    assert sum(len(v) for v in files.values()) > len(set(lines)) == len(lines) == 7
    assert all(sum(x in v for v in files.values()) >= 2 for x in lines)
    return {k: "".join(x + "\n" for x in v) for k, v in files.items()}


def write_inputs(folder):
    """-> (genome.fa, the align directory)"""
    fasta, align = os.path.join(folder, "genome.fa"), os.path.join(folder, "align")
    G.write_fasta(fasta, NAMES, genome(), WIDTHS)
    os.makedirs(align)
    for name, text in bucket_files().items():
        with open(os.path.join(align, name), "w") as f:
            f.write(text)
    with open(os.path.join(align, "bucket_0000.log"), "w") as f:  # (not an *.aligned.bed: left alone)
        f.write("chrZ\t1\t2\n")
    return fasta, align


def decimal_bucket():
    """A bucket whose first line has a decimal point in its start column (a number column the records do not take): the copy of
    COPIES[0] that `stats generate` reads as the same alignment (atoi), in front of two ordinary lines, one of them twice."""
    lines = [aligned_line(*COPIES[0]).replace("\t200\t", "\t200.5\t", 1), aligned_line(*COPIES[1]), aligned_line(*COPIES[0]), aligned_line(*COPIES[1])]
    assert lines[0].split("\t")[1] == "200.5"
    return "".join(x + "\n" for x in lines)
