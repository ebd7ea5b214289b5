"""Models and cases for the tests of sdf_seed_records and `sedef seeds`: the record of a search hit stated through its BED
text, the pairs of a run as the loops of sedef.sh (:133-140) state them, job tables with empty jobs at every place, and the
genome the command's test runs on."""
import numpy as np

import search_cmd_gen as G

I31 = 2 ** 31 - 1
SEED_RC = 1


def ids_of(names):
    """name -> id: the numbering of sdf_bucket_merge, byte order of the names."""
    return {nm: k for k, nm in enumerate(sorted(set(names), key=lambda s: s.encode()))}


def record_by_text(host, seeds, ids, qname, rname, hit, reverse, ref_len):
    """The sdf_seed_hit of a hit: Hit::from_bed of the line `sedef search` prints for it, both through the host library."""
    qs, qe, rs, re_ = (int(x) for x in hit)
    qn, a, b, rn, c, d, q_rc, r_rc = seeds.hit_from_bed(host.search_hit_bed(qname, rname, qs, qe, rs, re_, reverse, ref_len))
    assert not q_rc and r_rc == bool(reverse)
    return (ids[qn], a, b, ids[rn], c, d, SEED_RC if r_rc else 0, 0)


def records_by_text(host, seeds, names, hits, first, jobs):
    """... of every hit of a call: jobs = (query name, reference name, ref_len, reverse) rows; hit t belongs to the job whose
    range [first[j], first[j + 1]) holds it."""
    ids, out = ids_of(names), []
    for j, (qn, rn, ref_len, reverse) in enumerate(jobs):
        for t in range(int(first[j]), int(first[j + 1])):
            out.append(record_by_text(host, seeds, ids, qn, rn, hits[t], reverse, ref_len))
    return out


def job_rows(names, jobs):
    """(query name, reference name, ref_len, reverse) rows -> (q_chr, r_chr, ref_len, reverse) rows."""
    ids = ids_of(names)
    return [(ids[q], ids[r], n, int(bool(rv))) for q, r, n, rv in jobs]


def pairs_model(groups):
    """The pairs of a run: sedef.sh launches `sedef search [-r] -t i j` for j = 0 .., i = j .., m = n then y, and such a process
    runs `for r in group j, for q in group i` with same_genome = (q == r) and not reverse."""
    out = []
    for j in range(len(groups)):
        for i in range(j, len(groups)):
            for reverse in (False, True):
                for r in groups[j]:
                    for q in groups[i]:
                        out.append((i, j, reverse, q, r, q == r and not reverse))
    return out


# ---- job tables for the device forms: eight jobs -- the first empty, two empty ones in a row in the middle, the last empty, and
# (from n = 65) a boundary at hit 64 exactly ----
NAMES = ["chr1", "chr10", "chr2", "chrX"]
TABLE_JOBS = [("chr1", "chr1", 5000, False), ("chr2", "chr1", 90000, True), ("chr10", "chrX", I31, False), ("chrX", "chrX", 7, True),
              ("chr1", "chr10", 1, False), ("chrX", "chr2", I31, True), ("chr10", "chr10", 123456789, True), ("chr2", "chrX", 0, False)]
TABLE_SIZES = (0, 1, 63, 64, 65, 4097)


def table_first(n):
    c1, c2, c3 = min(n, 17), min(n, 64), min(n, 1000)
    return np.array([0, 0, c1, c2, c2, c2, c3, n, n], np.uint64)


def table_hits(n, seed=0):
    """n hits of any coordinates below 2^31 (the rule is arithmetic: flips that wrap are among them)."""
    rng = np.random.default_rng(1000 + seed + n)
    a = rng.integers(0, I31, (n, 4), dtype=np.int64)
    a[:, 1] = np.maximum(a[:, 0], a[:, 1])
    a[:, 3] = np.maximum(a[:, 2], a[:, 3])
    return a


# ---- the genome of the command's test: three records in two translation groups ([s1, s2] and [s3] at GROUP_LIMIT); copies inside
# s1, from s1 into s2 twice 200 bases apart (two SDs within merge_dist of each other), from s2 into s3, and an INVERTED one from s1
# into s3; lowercase stretches and an N run; the sizes of tests/test_gpu_search_cmd.py ----
GENOME_NAMES = ["s1", "s2", "s3"]
GENOME_LENS = [12000, 9000, 7000]
GENOME_COPIES = [(0, 500, 2500, 0, 7000, 0.05, False), (0, 3500, 1500, 1, 1000, 0.04, False), (0, 5200, 1500, 1, 2700, 0.04, False),
                 (1, 5000, 1800, 2, 3000, 0.08, False), (0, 9800, 1600, 2, 500, 0.03, True)]
GENOME_SEED = 5
GENOME_WIDTHS = [60, 70, 60]
GROUP_LIMIT = 22000  # (test-only, SDF_TEST_TRANSLATE_LIMIT)


def genome_records():
    return G.records(GENOME_SEED, GENOME_LENS, GENOME_COPIES, lower=[(0, 2000, 300), (1, 1200, 200)], n_runs=[(2, 6000, 150)])


def genome_groups():
    return G.translation_model(list(zip(GENOME_LENS, GENOME_NAMES)), GROUP_LIMIT)


def write_genome(path):
    G.write_fasta(path, GENOME_NAMES, genome_records(), GENOME_WIDTHS)
