"""The definition of the coverage call and of `sedef stats diff`, from the reference's get_differences
(src/stats_main.cc:397-509), Hit::from_bed / from_wgac (src/hit.cc:29-63, 99-118) and get_sequence's clamp
(src/fasta.cc:105-119): numpy boolean arrays, one per set and region; painting is slice assignment, the predicates are byte
comparisons, the seven counts np.count_nonzero.  Where the reference is undefined the model follows what the issue fixed:
WGAC coordinates are clamped to the chromosome, a chromosome WGAC never names has an empty WGAC set."""
import re

import numpy as np

COUNT_FIELDS = ("a", "b", "both", "a_only", "b_only", "a_only_upper", "b_only_upper")


def is_upper(chars):
    """isupper() in the C locale (:417, :421), on the whole byte: N and the IUPAC letters count, n and bytes >= 128 do not."""
    return (chars >= ord("A")) & (chars <= ord("Z"))


def is_upper_base(chars):
    """isupper(c) && toupper(c) != 'N' (:485, :488)."""
    return is_upper(chars) & (chars != ord("N"))


def coverage(pool, regions, intervals, min_upper):
    """pool: uint8 array; regions: (off, len); intervals: (region, start, len, set, partner).  Returns (counts: int64
    [n_regions, 7] in COUNT_FIELDS order, upper: int32 [n_iv], painted: uint8 [n_iv])."""
    pool = np.frombuffer(bytes(pool), np.uint8)
    chars = [pool[off:off + n] for off, n in regions]
    upper = np.array([np.count_nonzero(is_upper(chars[r][s:s + n])) for r, s, n, _, _ in intervals], np.int32).reshape(-1)
    painted = np.array([p < 0 or (upper[i] >= min_upper and upper[p] >= min_upper) for i, (_, _, _, _, p) in enumerate(intervals)],
                       np.uint8).reshape(-1)
    sets = [[np.zeros(n, bool) for _, n in regions] for _ in range(2)]
    for (r, s, n, which, _), go in zip(intervals, painted):
        if go:
            sets[which][r][s:s + n] = True
    counts = np.zeros((len(regions), 7), np.int64)
    for r in range(len(regions)):
        a, b, u = sets[0][r], sets[1][r], is_upper_base(chars[r])
        counts[r] = [np.count_nonzero(x) for x in (a, b, a & b, a & ~b, b & ~a, a & ~b & u, b & ~a & u)]
    return counts, upper, painted


def counts_rows(rec):
    """A COVER_COUNTS_DTYPE array as int64 [n, 7]."""
    return np.stack([rec[f] for f in COUNT_FIELDS], axis=1).astype(np.int64) if len(rec) else np.zeros((0, 7), np.int64)


def atoi(s):
    m = re.match(r"\s*([+-]?\d+)", s)
    return int(m.group(1)) if m else 0


def stats_diff_lines(chroms, bed_text, wgac_text, min_upper=100):
    """chroms: name -> bytes.  Returns (the nine lines `stats diff` prints, the seven figures)."""
    length = {k: len(v) for k, v in chroms.items()}
    sedef, wgac = {}, {}
    n_in = n_miss = 0
    for line in bed_text.split("\n"):
        if not line or line[0] == "#":
            continue
        ss = line.split("\t")
        assert len(ss) >= 10
        sides = []
        for name, s, e in ((ss[0], atoi(ss[1]), atoi(ss[2])), (ss[3], atoi(ss[4]), atoi(ss[5]))):
            e = min(e, length[name])              # get_sequence: *end > entry.length -> entry.length
            s0 = max(s, 0)                        # ... and a start below 0 reads from 0
            sides.append((name, s0, e, np.count_nonzero(is_upper(np.frombuffer(chroms[name][s0:max(e, s0)], np.uint8)))))
        if sides[0][3] < min_upper or sides[1][3] < min_upper:
            n_miss += 1
            continue
        n_in += 1
        for name, s, e, _ in sides:
            sedef.setdefault(name, np.zeros(length[name], bool))[s:e] = True
    seen = set()
    for line in wgac_text.split("\n")[1:]:
        if not line:
            continue
        ss = line.split("\t")
        assert len(ss) >= 27
        if len(ss[0]) > 6 or len(ss[6]) > 6 or ss[16] in seen:
            continue
        seen.add(ss[16])
        for name, s, e in ((ss[0], atoi(ss[1]), atoi(ss[2])), (ss[6], atoi(ss[7]), atoi(ss[8]))):
            if name in length:
                s, e = min(max(s, 0), length[name]), min(max(e, 0), length[name])
                wgac.setdefault(name, np.zeros(length[name], bool))[s:e] = True
    t = np.zeros(7, np.int64)
    for name, a in sedef.items():
        b = wgac.get(name, np.zeros(length[name], bool))
        u = is_upper_base(np.frombuffer(chroms[name], np.uint8))
        t += [np.count_nonzero(x) for x in (a, b, a & b, a & ~b, b & ~a, a & ~b & u, b & ~a & u)]
    a, b, both, a_only, b_only, a_up, b_up = (int(x) for x in t)
    lines = ["SEDEF reading done (in %d, miss %d)!" % (n_in, n_miss), "WGAC reading done!",
             "SEDEF: spans              %12d" % a, "       unique             %12d" % a_only, "       unique (uppercase) %12d" % a_up,
             "       misses             %12d" % b_only, "       misses (uppercase) %12d" % b_up, "WGAC:  spans              %12d" % b,
             "       intersects         %12d" % both]
    return lines, (a, a_only, a_up, b_only, b_up, b, both)
