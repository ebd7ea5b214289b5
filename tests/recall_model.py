"""The definition of the pair-recall call (include/sedef_hip.h: sdf_pair_recall) and of `sedef stats recall`
(csrc/host/stats_recall.cc), from the rule alone: every gold record against every found record, a painted numpy array per side.
`bedtools pairtopair -type both`, which the reference's scratch/check-overlap.py leaves the join to, is no part of this build;
this file and the header are the project's statement of it.

A record is a row (chr1, start1, end1, chr2, start2, end2, flags[, reserved]); bit 0 of flags is the strand of end 1, bit 1 that
of end 2.  Nothing here is sorted, binned or capped: the cap only decides the WIDE flag."""
import numpy as np

IGNORE_STRAND = 1
WIDE = 1
ERR_UNSUPPORTED, ERR_INVALID = -3, -4


def bad_record(r):
    r = list(r) + [0] * (8 - len(r))
    return r[0] < 0 or r[3] < 0 or r[1] < 0 or r[4] < 0 or r[1] > r[2] or r[4] > r[5] or r[7] != 0 or (r[6] & ~3) != 0


def refusal(gold, found, flags):
    """The code the host forms answer instead of a result, or 0."""
    if flags & ~IGNORE_STRAND:
        return ERR_UNSUPPORTED
    if any(bad_record(r) for r in gold) or any(bad_record(r) for r in found):
        return ERR_INVALID
    return 0


def _columns(rows):
    a = np.asarray([list(r)[:7] for r in rows], dtype=np.int64).reshape(-1, 7)
    ends = ((a[:, 0], a[:, 1], a[:, 2], a[:, 6] & 1), (a[:, 3], a[:, 4], a[:, 5], (a[:, 6] >> 1) & 1))
    return ends


def _meets(g, f, ignore):
    """End g (scalars) against the ends f (arrays): same chromosome, at least one common base, equal strands."""
    return (f[0] == g[0]) & (np.minimum(f[2], g[2]) - np.maximum(f[1], g[1]) >= 1) & (ignore | (f[3] == g[3]))


def pair_recall(gold, found, flags=0, cap=1024):
    """-> [(n_hits, cov1, cov2, flags)] per gold record."""
    assert refusal(gold, found, flags) == 0
    ignore = bool(flags & IGNORE_STRAND)
    f1, f2 = _columns(found)
    out = []
    for r in gold:
        g1, g2 = (r[0], r[1], r[2], r[6] & 1), (r[3], r[4], r[5], (r[6] >> 1) & 1)
        direct = _meets(g1, f1, ignore) & _meets(g2, f2, ignore)
        cross = _meets(g1, f2, ignore) & _meets(g2, f1, ignore)
        paint1, paint2 = np.zeros(g1[2] - g1[1], bool), np.zeros(g2[2] - g2[1], bool)

        def paint(arr, g, f, i):
            arr[max(int(f[1][i]), g[1]) - g[1]:min(int(f[2][i]), g[2]) - g[1]] = True
        for i in np.flatnonzero(direct):
            paint(paint1, g1, f1, i)
            paint(paint2, g2, f2, i)
        for i in np.flatnonzero(cross):
            paint(paint1, g1, f2, i)
            paint(paint2, g2, f1, i)
        listed = int(direct.sum()) + int(cross.sum())
        out.append((int((direct | cross).sum()), int(paint1.sum()), int(paint2.sum()), WIDE if listed > cap else 0))
    return out


def listed(gold_row, found, flags=0):
    """The direct and crosswise hits of one gold record together: what the cap is held against."""
    ignore = bool(flags & IGNORE_STRAND)
    f1, f2 = _columns(found)
    r = gold_row
    g1, g2 = (r[0], r[1], r[2], r[6] & 1), (r[3], r[4], r[5], (r[6] >> 1) & 1)
    return int((_meets(g1, f1, ignore) & _meets(g2, f2, ignore)).sum()) + int((_meets(g1, f2, ignore) & _meets(g2, f1, ignore)).sum())


# ---- `sedef stats recall` ------------------------------------------------------------------------------------------------------

def _commas(v):
    return "{:,}".format(v)


def _c_round(x):
    """C's round(): halves away from zero (python2's round)."""
    return float(np.floor(abs(x) + 0.5)) * (1 if x >= 0 else -1)


def stats_recall_text(bed_text, wgac_text, ignore_strand=False, cap=1024):
    """-> (the text of out.txt, the four stdout lines as one string, rows with an empty side skipped)."""
    ids = {}

    def cid(name):
        return ids.setdefault(name, len(ids))
    found = []
    for ln in bed_text.split("\n"):
        if not ln or ln.startswith("#"):
            continue
        ss = ln.split("\t")
        found.append((cid(ss[0]), int(ss[1]), int(ss[2]), cid(ss[3]), int(ss[4]), int(ss[5]), (ss[8][:1] != "+") | ((ss[9][:1] != "+") << 1)))
    gold, rows, names, data_lines, empty = [], [], {}, 0, 0
    for ln in wgac_text.split("\n")[1:]:
        if not ln:
            continue
        ss = ln.split("\t")
        data_lines += 1
        if "_" in ss[0] or "_" in ss[6]:
            continue
        s1, e1, s2, e2 = int(ss[1]), int(ss[2]), int(ss[7]), int(ss[8])
        if s1 == e1 or s2 == e2:
            empty += 1
            continue
        names.setdefault(ss[16], []).append(len(gold))
        gold.append((cid(ss[0]), s1, e1, cid(ss[6]), s2, e2, 2 if ss[5] == "_" else 0))
        rows.append((ss[0], s1, e1, ss[6], s2, e2, ss[5]))
    rec = pair_recall(gold, found, IGNORE_STRAND if ignore_strand else 0, cap)
    out, partial, missed, full = [], [], 0, 0
    for name in sorted(names, key=lambda s: s.encode()):
        of = names[name]
        hit = [g for g in of if rec[g][0]]
        if not hit:
            missed += 1
            r = rows[of[-1]]
            out.append("MISS\t%s\t%d\t%d\t%s\t%d\t%d\t%s\tlen1=%s\tlen2=%s\thttp://humanparalogy.gs.washington.edu/build37/%s" %
                       (r[0], r[1], r[2], r[3], r[4], r[5], r[6], _commas(r[2] - r[1]), _commas(r[5] - r[4]), name))
            continue
        g = hit[0]
        p1, p2 = rec[g][1] / float(gold[g][2] - gold[g][1]), rec[g][2] / float(gold[g][5] - gold[g][4])
        if _c_round(p1 * 100) < 80 or _c_round(p2 * 100) < 80:
            partial.append((p1 + p2, name.encode(), p1, p2, name))
        else:
            full += 1
    for _, _, p1, p2, name in sorted(partial):
        out.append("PART\t%.2f\t%.2f\thttp://humanparalogy.gs.washington.edu/build37/%s" % (p1 * 100, p2 * 100, name))
    n = len(names)

    def pct(v):
        return 100.0 * v / n if n else 0.0
    report = "WGAC:     {:>6} ({} lines)\n".format(_commas(n), _commas(data_lines))
    report += "Missed:  {:>7} hits ({:4.1f}%)\n".format(_commas(missed), pct(missed))
    report += "Partial: {:>7} hits ({:4.1f}%)\n".format(_commas(len(partial)), pct(len(partial)))
    report += "Full:    {:>7} hits ({:4.1f}%)\n".format(_commas(full), pct(full))
    return "".join(x + "\n" for x in out), report, empty
