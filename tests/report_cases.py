"""The case lines of the line-order tests (tests/test_line_order_cpu.py, tests/test_gpu_line_order.py): name -> list of lines
(bytes, no newline), each table small enough to order in well under a second, each edge asserted where it is built.  `expected`
is what tests/report_model.py makes of a table, computed once."""
import functools
import random

import report_model as M

STEP = 1024  # bytes of two lines the tie kernel compares in one step (line_order.hip)
NAMES = [b"chr1", b"chr2", b"chr10", b"chr17", b"chr17_ctg5_hap1", b"chr1_gl000191_random", b"chrM", b"chrUn_gl000211", b"chrX"]
NAMES_SORTED = [b"chr1", b"chr1_gl000191_random", b"chr2", b"chr10", b"chr17", b"chr17_ctg5_hap1", b"chrM", b"chrUn_gl000211", b"chrX"]


def bed(c1, s1, e1, c2, s2, e2, name=b"", score=b"0.0", st1=b"+", st2=b"+", rest=(b"100", b"95", b"10M")):
    """A line of `align generate` / `stats generate`: an empty name leaves two tabs in a row, which sort reads as ONE run of blanks."""
    f = [c1, b"%d" % s1 if isinstance(s1, int) else s1, b"%d" % e1 if isinstance(e1, int) else e1, c2,
         b"%d" % s2 if isinstance(s2, int) else s2, b"%d" % e2 if isinstance(e2, int) else e2, name, score, st1, st2] + list(rest)
    return b"\t".join(f)


def padded(length, last=b"a", fill=b"N"):
    """A line of `length` bytes whose eight keys do not depend on `last` or `fill`: six columns and a seventh that takes the rest."""
    head = b"c\t1\t2\td\t3\t4\t"
    assert length > len(head) and len(last) == 1
    line = head + fill * (length - len(head) - 1) + last
    assert len(line) == length
    return line


def run_lengths(lines):
    """The lengths of the runs of equal keys, in sorted order."""
    order, _, _ = M.line_order(lines)
    out, p = [], 0
    while p < len(order):
        hi = p + 1
        while hi < len(order) and M.key_cmp(lines[order[p]], lines[order[hi]]) == 0:
            hi += 1
        out.append(hi - p)
        p = hi
    return out


def _sized(n, seed):
    """n lines of a few chromosomes and places, a third of them copies of an earlier line, shuffled."""
    rng = random.Random(seed)
    lines = []
    while len(lines) < n:
        if lines and rng.random() < 0.33:
            lines.append(rng.choice(lines))
            continue
        name = rng.choice([b"", b"", b"S"])
        lines.append(bed(rng.choice(NAMES), rng.randrange(40), rng.randrange(40, 90), rng.choice(NAMES), rng.randrange(5), rng.randrange(5, 9), name,
                         st1=rng.choice([b"+", b"-"]), st2=rng.choice([b"+", b"-"]), rest=(b"%d" % rng.randrange(3), b"M" * rng.randrange(1, 40))))
    rng.shuffle(lines)
    return lines


def _run(m, c1, seed):
    """m lines that share all eight keys and differ behind them, some of them twice, in no order."""
    rng = random.Random(seed)
    distinct = [bed(c1, 5, 50, b"chr2", 7, 70, b"S", rest=(b"%d" % k, b"M" * (1 + k % 7))) for k in range(max(1, m - m // 4))]
    lines = distinct + [rng.choice(distinct) for _ in range(m - len(distinct))]
    rng.shuffle(lines)
    assert len(lines) == m
    return lines


@functools.lru_cache(maxsize=None)
def tables():
    T = {}
    for n in (0, 1, 255, 256, 257):
        T["size_%d" % n] = _sized(n, n)
        assert len(T["size_%d" % n]) == n
    # runs of every length around the tie kernel's 64, each on a chromosome of its own, dealt into one another
    runs = [_run(m, b"chr%d" % m, m) for m in (1, 2, 63, 64, 65)]
    mixed = [x for r in runs for x in r]
    random.Random(5).shuffle(mixed)
    T["run_lengths"] = mixed
    assert sorted(run_lengths(mixed)) == [1, 2, 63, 64, 65]
    T["run_of_64_alone"] = _run(64, b"chr1", 64)
    T["run_of_65_alone"] = _run(65, b"chr1", 65)
    assert run_lengths(T["run_of_64_alone"]) == [64] and run_lengths(T["run_of_65_alone"]) == [65]
    T["two_wide_runs_side_by_side"] = _run(70, b"chr1", 1) + _run(66, b"chr2", 2)
    assert run_lengths(T["two_wide_runs_side_by_side"]) == [70, 66]
    # line lengths around the 16 bytes of a lane and the 1 KiB of a step; every length: the line, a copy, one that differs in the
    # last byte and one a byte longer (the line is its prefix)
    lengths = []
    for length in (15, 16, 17, 1023, 1024, 1025, 2049):
        lengths += [padded(length, b"b"), padded(length, b"a"), padded(length, b"b"), padded(length, b"b") + b"x"]
    T["line_lengths"] = [b"a", b"b", b"a"] + lengths + [b""]
    assert sorted({len(x) for x in T["line_lengths"]}) == [0, 1, 15, 16, 17, 18, 1023, 1024, 1025, 1026, 2049, 2050]
    assert run_lengths(lengths) == [len(lengths)]
    T["last_byte"] = [padded(n, b"z") for n in (40, 1024, 2048)] + [padded(n, b"y") for n in (40, 1024, 2048)]
    # the first byte of a new step: bytes 1024 and 2048 of lines that agree everywhere else
    base = padded(3000)
    at_step = [base[:k] + b"M" + base[k + 1:] for k in (STEP, 2 * STEP)] + [base, base[:STEP - 1] + b"M" + base[STEP:]]
    T["first_byte_of_a_step"] = at_step
    assert run_lengths(at_step) == [4] and len(set(at_step)) == 4
    T["prefixes"] = [padded(20) + b"Q" * k for k in (3, 0, 1100, 1, 1024, 0)]
    # unsigned bytes: 0x80 and 0xff sort behind 0x7f and 0x01
    T["high_bytes"] = [padded(50, bytes([c])) for c in (0x80, 0x7F, 0xFF, 0x01)] + [padded(1500, b"a", bytes([c])) for c in (0xC3, 0x41, 0x80)]
    assert M.sort_uniq(T["high_bytes"][:4]) == [padded(50, bytes([c])) for c in (0x01, 0x7F, 0x80, 0xFF)]
    same = bed(b"chr2", 10, 20, b"chr3", 30, 40, b"S", rest=(b"12", b"5M"))
    T["three_identical_spread"] = [same, bed(b"chr1", 1, 2, b"chr1", 3, 4, b"S"), bed(b"chr2", 10, 20, b"chr3", 30, 40, b"S", rest=(b"11", b"5M")), same,
                                   bed(b"chrX", 1, 2, b"chr1", 3, 4, b"S"), bed(b"chr2", 10, 21, b"chr3", 30, 40, b"S"), same]
    assert M.line_order(T["three_identical_spread"])[2] == 5
    T["only_k6_differs"] = [bed(b"chr1", 10, 20, b"chr2", 30, e2, b"S") for e2 in (41, 40, 100, 9, 40)]
    T["only_k1_differs"] = [bed(c1, 10, 20, b"chr2", 30, 40, b"S") for c1 in reversed(NAMES)]
    assert [M.field(x, 1) for x in M.sort_uniq(T["only_k1_differs"])] == NAMES_SORTED
    # the field shift: without a name, "field 9" is the second strand and "field 10" the column behind it
    shift = [bed(b"chr1", 10, 20, b"chr2", 30, 40, name, st1=a, st2=b, rest=(r, b"3M")) for name in (b"", b"S") for a in (b"+", b"-")
             for b in (b"+", b"-") for r in (b"7", b"9")]
    T["empty_name_mixed"] = shift
    assert M.field(shift[0], 9) == b"\t+" and M.field(shift[0], 10) == b"\t7" and M.field(shift[-1], 9) == b"\t-" and M.field(shift[-1], 10) == b"\t-"
    header = b"#chr1\tstart1\tend1\tchr2\tstart2\tend2\tname\tscore\tstrand1\tstrand2\tmax_len\taln_len"
    T["header_line"] = [bed(b"chr1", 10, 20, b"chr2", 30, 40, b"S"), header, bed(b"chrM", 1, 2, b"chr1", 3, 4, b"S"), header]
    assert M.sort_uniq(T["header_line"])[-1] == header  # (version order: '#' sorts behind the letters, so the header ends the file)
    T["n_field_without_digits"] = [bed(b"chr1", s1, 20, b"chr2", 30, 40, b"S") for s1 in (b"5", b"x", b"0", b"", b"007", b"7", b"12abc")]
    assert M.plain(T["n_field_without_digits"]) and M.number(b"\tx") == 0 and M.number(b"\t12abc") == 12
    T["decimal_point"] = [bed(b"chr1", s1, 20, b"chr2", 30, 40, b"S") for s1 in (b"5", b"4.5", b"4.50", b"-3", b".5", b"4.25", b"10", b"-0")]
    assert not M.plain(T["decimal_point"])
    T["too_large_for_a_value"] = [bed(b"chr1", s1, 20, b"chr2", 30, 40, b"S") for s1 in (b"4294967296", b"4294967295", b"00000000001", b"1")]
    assert not M.plain(T["too_large_for_a_value"]) and M.plain(T["too_large_for_a_value"][1:2])
    return T


@functools.lru_cache(maxsize=None)
def expected(name):
    """(order, flags, n_kept) of a table, by the model."""
    return M.line_order(tables()[name])


def wide_only_on_long_runs(lines, order, flags):
    """WIDE on every place of a run of more than RUN lines and nowhere else."""
    p = 0
    while p < len(order):
        hi = p + 1
        while hi < len(order) and M.key_cmp(lines[order[p]], lines[order[hi]]) == 0:
            hi += 1
        if any(bool(flags[q] & M.WIDE) != (hi - p > M.RUN) for q in range(p, hi)):
            return False
        p = hi
    return True
