"""Case tables for the three ways stats_cols.hip counts an alignment, and the rule that chooses between them.

The kernel decides per quad of four consecutive tasks (stats_columns_kernel): all four at most `group_max` runs -> one
wavefront takes them in its four rows of sixteen lanes, sixteen runs a chunk (stats_count_groups); else every task gets a
wavefront of its own, 64 runs a chunk (stats_count_alignment), and one of more than STATS_LONG runs is cut into segments of
STATS_SEG runs.  paths() states that rule; cells() says which edges of those paths a batch reaches, and every table carries
the cells it is meant to reach -- tests/test_stats_paths_cpu.py holds the tables to that without a GPU, so that
tests/test_gpu_stats_paths.py cannot go hollow.  Nothing here computes an expected counter: those come from
oracle/stats_oracle.c.

A case is (a, b, runs): the two sides as bytes and runs = [(op, len)], op 0 'M', 1 'D' (a only), 2 'I' (b only).
A spec (the resident form) is (a_off, a_len, b_off, b_len, runs, a_rc, b_rc) over POOL, as in tests/test_gpu_stats_resident.py."""
import itertools

import numpy as np

GROUP_MAX, SEG, LONG = 32, 512, 1024  # STATS_GROUP_MAX (extz2_geom.h), STATS_SEG, STATS_LONG (stats_cols.hip)
M, D, I = 0, 1, 2
RUN_COUNTS = (0, 1, 15, 16, 17, 31, 32)  # runs of a row: nothing, one, around the first chunk's end, around the second's
RUN_LENS = (1, 7, 8, 9, 15, 16, 17)  # columns of a run: around one and two units of eight
UNIT_TOTALS = (0, 1, 15, 16, 17, 33)  # units of a row's chunk: around one round of sixteen, and into a third
WHOLE_COUNTS = (33, 63, 64, 65, 127, 128, 129, 1023, 1024)
WHOLE_UNITS = (63, 64, 65, 127, 128, 129, 191, 192, 193)  # units of a 64-run chunk: the `two` branch, the 128-unit round
SEGMENT_COUNTS = (1025, 1536, 1537)


def paths(n_cigars, group_max=GROUP_MAX):
    """The path of every task of a batch, in order: 'group', 'whole' or 'segments'."""
    n = [int(c) for c in n_cigars]
    out = []
    for task, c in enumerate(n):
        quad = n[task & ~3:(task & ~3) + 4]  # (the present tasks of the quad: a batch's tail has fewer than four)
        if group_max != 0 and max(quad) <= group_max:
            out.append("group")
        else:
            out.append("segments" if c > LONG else "whole")
    return out


def words(runs):
    return np.array([(l << 4) | op for op, l in runs], np.uint32)


def need(runs):
    """The bases of a and of b that the runs consume."""
    return sum(l for op, l in runs if op != I), sum(l for op, l in runs if op != D)


def _units(l):
    return (l + 7) >> 3


# ---- sequences ---------------------------------------------------------------------------------------------------------------
def _material(n, seed):
    """Mixed case in soft-masked stretches of 3..39, N / n runs every 151 bytes, one byte >= 0x80 every 263."""
    rng = np.random.default_rng(seed)
    s = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].copy()
    pos, lo = 0, False
    while pos < n:
        step = int(rng.integers(3, 40))
        if lo:
            s[pos:pos + step] |= 0x20
        pos, lo = pos + step, not lo
    for p in range(37, n, 151):
        s[p:p + 1 + p % 5] = ord("N") if p % 2 else ord("n")
    for p in range(101, n, 263):
        s[p] = 0x80 + (7 * p) % 128
    return s


BASE = _material(1 << 16, 20260)
POOL = BASE[:12007].copy()  # the resident pool of the strand and segment tables (its length is no multiple of eight)


def rev_table():
    """rev_dna of the reference (src/common.h:72-87,93): ACGT of either case complemented, everything else 'N', indexed c & 127."""
    tab = np.full(128, ord("N"), np.uint8)
    for x, y in zip(b"ACGTacgt", b"TGCAtgca"):
        tab[x] = y
    return np.concatenate([tab, tab])


def aln(runs, salt=0, spare_a=0, spare_b=0):
    """A case for `runs`: a from BASE, b follows a along the M runs with a substitution every ninth base and a flipped case
    every seventh letter; spare_a / spare_b bases lie behind what the runs consume."""
    runs = [(int(op), int(l)) for op, l in runs]
    na, nb = need(runs)
    na, nb = na + spare_a, nb + spare_b
    start = (salt * 131) % 20000
    a = BASE[start:start + na].copy()
    b = BASE[30000 + start:30000 + start + nb].copy()
    ia = ib = 0
    for op, l in runs:
        if op == M:
            b[ib:ib + l] = a[ia:ia + l]
        ia += l if op != I else 0
        ib += l if op != D else 0
    k = np.arange(nb) + salt
    sub = k % 9 == 0
    b[sub] = np.frombuffer(b"ACGT", np.uint8)[k[sub] % 4]
    letter = ((b & 0xDF) >= ord("A")) & ((b & 0xDF) <= ord("Z")) & (b < 0x80)
    b[letter & (k % 7 == 3)] ^= 0x20
    return a.tobytes(), b.tobytes(), runs


def row(n_runs, salt, lens=RUN_LENS):
    """A row of n_runs runs: ops M D M I M ... and lengths from `lens`, both turned by `salt`."""
    return aln([((M, D, M, I, M)[(k + salt) % 5], lens[(3 * k + salt) % len(lens)]) for k in range(n_runs)], salt,
               spare_a=salt % 3, spare_b=salt % 2)


# ---- which edges a batch reaches ------------------------------------------------------------------------------------------------
def _zero_kinds(runs):
    n, kinds = len(runs), set()
    zero = [k for k, (_, l) in enumerate(runs) if l == 0]
    if not zero:
        return kinds
    if len(zero) == n:
        kinds.add("only")
    else:
        if 0 in zero:
            kinds.add("first")
        if n - 1 in zero:
            kinds.add("last")
        if any(0 < k < n - 1 and runs[k - 1][1] > 0 and runs[k + 1][1] > 0 for k in zero):
            kinds.add("between")
    for k in (15, 16):  # the last run of a row's first chunk, the first of its second
        if k in zero and n > 17:
            kinds.add(("at", k))
    for k in zero:
        if runs[k][0] != M:
            kinds.add("zero_D" if runs[k][0] == D else "zero_I")
    return kinds


def cells(batch, group_max=GROUP_MAX):
    """The edges that one call on `batch` reaches, by the path that paths() gives every task."""
    n = [len(c[2]) for c in batch]
    ps = paths(n, group_max)
    hit = {("batch_tasks", len(batch))}
    for q0 in range(0, len(batch), 4):
        rows, counts = batch[q0:q0 + 4], tuple(n[q0:q0 + 4])
        if ps[q0] != "group":
            continue
        hit.add(("group_quad", counts))
        if len(rows) < 4:
            hit.add(("group_tail", len(rows)))
        for pos, c in enumerate(counts):
            hit.add(("group_runs", c, pos))
        if len(rows) == 4 and sum(c > 16 for c in counts) == 1:
            hit.add("group_one_row_in_second_chunk")
        if len({-(-c // 16) for c in counts}) > 1:
            hit.add("group_rows_end_in_different_chunks")
        for base in range(0, max(counts), 16):
            rounds = set()
            for _, _, runs in rows:
                u = sum(_units(l) for _, l in runs[base:base + 16])
                rounds.add(-(-u // 16))
                if len(runs) > base:
                    hit.add(("group_chunk_units", u))
            if len(rounds) > 1:
                hit.add("group_rows_end_in_different_rounds")
        wide = [len(a) >= 8 or len(b) >= 8 for a, b, _ in rows]
        for r, (a, b, runs) in enumerate(rows):
            na, nb = need(runs)
            for kind in _zero_kinds(runs):
                hit.add(("group_zero", kind))
            for _, l in runs:
                hit.add(("group_run_len", l))
            for side, s in (("a", a), ("b", b)):
                if len(s) < 8 and any(w for k, w in enumerate(wide) if k != r):
                    hit.add(("group_narrow_side", side, len(s)))
            if na + nb > 0:
                hit.add(("group_stops_short", len(a) - na, len(b) - nb))
            if len(a) == 8 == na:
                hit.add(("group_side_of_8", "a"))
            if len(b) == 8 == nb:
                hit.add(("group_side_of_8", "b"))
    for task, (a, b, runs) in enumerate(batch):
        if ps[task] == "whole":
            hit.add(("whole_runs", len(runs)))
            hit.add(("whole_at_row", len(runs), task & 3))
            for base in range(0, len(runs), 64):
                hit.add(("whole_chunk_units", sum(_units(l) for _, l in runs[base:base + 64])))
            for k in (63, 64):  # the last run of the first chunk, the first of the second
                if len(runs) > 65 and runs[k][1] == 0:
                    hit.add(("whole_zero_at", k))
        elif ps[task] == "segments":
            hit.add(("segments_runs", len(runs)))
            for base in range(0, len(runs), SEG):
                da, db = need(runs[base:base + SEG])
                if da == 0 and db > 0:
                    hit.add("segment_without_a")
                if db == 0 and da > 0:
                    hit.add("segment_without_b")
    return hit


class Table:
    """batches: every batch is one call.  want: {group_max: cells that the batches together must reach under it}."""

    def __init__(self, name, batches, want):
        self.name, self.batches, self.want = name, batches, want

    def missing(self, group_max=GROUP_MAX):
        hit = set().union(*(cells(b, group_max) for b in self.batches))
        return sorted(self.want.get(group_max, set()) - hit, key=repr)


# ---- 2. the grouped path ------------------------------------------------------------------------------------------------------------
def _runs_table():
    quads = [tuple(RUN_COUNTS[(i + p) % 7] for p in range(4)) for i in range(7)]  # every count in every row position
    quads += list(itertools.permutations((0, 1, 16, 32)))
    quads += [(32, 0, 0, 0), (0, 0, 0, 17)]  # (only one row has runs at all; only the last reaches the second chunk)
    batch = [row(c, 4 * q + p) for q, quad in enumerate(quads) for p, c in enumerate(quad)]
    want = {("group_runs", c, pos) for c in RUN_COUNTS for pos in range(4)}
    want |= {("group_quad", q) for q in quads}
    want |= {"group_one_row_in_second_chunk", "group_rows_end_in_different_chunks"}
    want |= {("group_run_len", l) for l in RUN_LENS}
    return Table("runs per row", [batch], {GROUP_MAX: want})


def _ops(lens, salt):
    return [((M, D, M, I, M)[(k + salt) % 5], l) for k, l in enumerate(lens)]


def _units_table():
    u33_1 = aln(_ops([16] * 15 + [17] + [1], 0), 1)  # 33 units (a third round), then 1
    u1_33 = aln(_ops([1] + [0] * 15 + [17] * 11, 1), 2)  # 1 unit, then 33
    u16_17 = aln(_ops([8] * 16 + [1] * 15 + [9], 2), 3)  # exactly one round, then one unit into the second
    u15_0 = aln(_ops([1, 7, 8] * 5 + [0] + [0, 0, 0], 3), 4)  # one unit short of a round, then a chunk of no units
    u17 = aln(_ops([17] * 5 + [9], 4), 5)
    one = [aln([(M, 1)], 6), aln([(D, 1)], 7), aln([(I, 1)], 8)]
    wide = aln([((M, D, I)[k % 3], 39) for k in range(16)], 9)  # sixteen runs of five units: five rounds beside one
    batch = [u33_1, u1_33, u16_17, u15_0,
             u15_0, u17, u1_33, u33_1,
             one[0], wide, one[1], one[2]]
    want = {("group_chunk_units", u) for u in UNIT_TOTALS + (80,)}
    want |= {"group_rows_end_in_different_rounds", "group_rows_end_in_different_chunks", ("group_quad", (1, 16, 1, 1))}
    return Table("units per row and chunk", [batch], {GROUP_MAX: want})


def _zero_table():
    body = [(M, 9), (D, 3), (M, 8), (I, 2), (M, 17)]
    lens20 = [(1, 7, 8, 9)[k % 4] for k in range(20)]

    def seam(at, n=20, salt=0):
        lens = [(1, 7, 8, 9)[k % 4] for k in range(n)]
        for k in at:
            lens[k] = 0
        return aln(_ops(lens, salt), 20 + salt)

    batch = [aln([(M, 0)] + body, 11), aln(body + [(I, 0)], 12), aln([(M, 8), (D, 0), (M, 8)], 13), aln([(M, 0), (D, 0), (I, 0)], 14, 5, 9),
             seam([15]), seam([16], salt=1), seam([15, 16], 32, 2), aln([(D, 0), (M, 0)], 15),  # (the last: no sequence at all)
             aln([(D, 0)] + body + [(M, 0)], 16), aln(_ops(lens20, 3), 17), aln([(M, 16), (I, 0), (D, 0), (M, 1)], 18), aln([(I, 0)], 19, 8, 0)]
    kinds = ["first", "last", "between", "only", ("at", 15), ("at", 16), "zero_D", "zero_I"]
    return Table("zero-length runs", [batch], {GROUP_MAX: {("group_zero", k) for k in kinds}})


def _lengths_table():
    batch = []
    for n in range(8):  # a side of 0..7 bytes (the narrow fetch) in a quad with rows of eight and more
        quad = [aln([(M, n), (I, 12 - n)], 30 + n), row(17 + n, 40 + n), aln([(M, n), (D, 12 - n)], 50 + n),
                aln([(M, n)], 60 + n) if n % 2 else aln([(M, max(n - 1, 0))], 60 + n, n - max(n - 1, 0), 0)]
        batch += quad[n % 4:] + quad[:n % 4]
    body = [(M, 17), (D, 2), (M, 9), (I, 3), (M, 8)]
    batch += [aln(body, 70), aln(body, 71, 1, 1), aln(body, 72, 9, 9), aln(body, 73, 1, 9),
              aln([(M, 8)], 74), aln([(M, 8), (I, 5)], 75), aln([(D, 3), (M, 8)], 76), aln(body, 77, 9, 0)]
    want = {("group_narrow_side", s, n) for s in "ab" for n in range(8)}
    want |= {("group_stops_short", d, d) for d in (0, 1, 9)} | {("group_side_of_8", "a"), ("group_side_of_8", "b")}
    return Table("sequence lengths", [batch], {GROUP_MAX: want})


def _tails_table():
    rows = [row(32, 80), row(1, 81), row(17, 82), row(16, 83), row(0, 84), row(31, 85), aln([(M, 3)], 86)]
    batches = [rows[k:k + n] for k, n in ((0, 1), (1, 2), (0, 3), (2, 5), (0, 6), (0, 7))]
    want = {("batch_tasks", n) for n in (1, 2, 3, 5, 6, 7)} | {("group_tail", n) for n in (1, 2, 3)}
    return Table("batch tails", batches, {GROUP_MAX: want})


def quad_rule_batches():
    """A quad of short alignments between two others; each of its positions in turn holds an alignment of 33 runs."""
    before = [row(c, 90 + p) for p, c in enumerate((16, 32, 1, 17))]
    quad = [row(c, 94 + p) for p, c in enumerate((31, 0, 32, 15))]
    after = [row(c, 98 + p) for p, c in enumerate((32, 17, 16, 32))]
    return [before + quad[:pos] + [row(33, 102 + pos)] + quad[pos + 1:] + after for pos in range(4)]


def _quad_rule_table():
    want = {("whole_at_row", 33, pos) for pos in range(4)} | {("whole_at_row", c, pos) for pos, c in enumerate((31, 0, 32, 15))}
    return Table("quad rule", quad_rule_batches(), {GROUP_MAX: want})


def _group_max_table():
    short = (1, 2, 3, 4, 5, 6, 7, 8, 9)
    counts = [(48, 49, 63, 64), (64, 1, 16, 48), (17, 65, 32, 0), (16, 16, 15, 0), (17, 1, 1, 1), (63, 64, 49, 17)]
    batch = [row(c, 110 + 4 * q + p, short) for q, quad in enumerate(counts) for p, c in enumerate(quad)]
    grouped = lambda quads: {("group_quad", q) for q in quads}  # noqa: E731
    whole = lambda cs: {("whole_runs", c) for c in cs}  # noqa: E731
    want = {GROUP_MAX: grouped(counts[3:5]) | whole((48, 49, 63, 64, 65, 17, 32, 0)),
            0: whole(c for quad in counts for c in quad),
            16: grouped(counts[3:4]) | whole((17, 1, 48, 65)),
            64: grouped(counts[:2] + counts[3:]) | whole((17, 65, 32, 0))}
    return Table("group_max", [batch], want)


GROUP_TABLES = [_runs_table(), _units_table(), _zero_table(), _lengths_table(), _tails_table(), _quad_rule_table(), _group_max_table()]
GROUP_MAX_SETTINGS = (None, 0, 16, 64)  # SDF_STATS_GROUP_MAX of the engines that run them (None: unset)


# ---- 2, strands: the resident form ------------------------------------------------------------------------------------------------
def sides(tab, pool, spec):
    """The two sides of a spec as the kernel reads them: a reversed side complemented on the host."""
    ao, al, bo, bl, _, a_rc, b_rc = spec
    a, b = pool[ao:ao + al], pool[bo:bo + bl]
    return (tab[a[::-1]] if a_rc else a).tobytes(), (tab[b[::-1]] if b_rc else b).tobytes()


def as_cases(specs, tab=None, pool=POOL):
    tab = rev_table() if tab is None else tab
    return [sides(tab, pool, s) + (s[4],) for s in specs]


def strand_specs():
    """Per quad the four strand combinations, turned over the row positions; rows of 17..32 runs and sides of 0..7 bytes; in
    every quad one a and one b range start at the pool's byte 0 and one of each end at its last byte."""
    P, specs = len(POOL), []
    for rot in range(4):
        for kind in range(3):
            for p in range(4):
                strand = (p + rot) % 4
                if kind == 0:
                    runs = row((17, 24, 31, 32)[(p + rot) % 4], 4 * rot + p)[2]
                elif kind == 1:
                    n = (2 * rot + p) % 8  # a side of n bytes
                    runs = [(M, n), (I if p % 2 else D, 11 + rot)]
                else:
                    n = 7 - (2 * rot + p) % 8
                    runs = [(I if p % 2 else D, 9), (M, n), (I if p % 2 else D, 0)]
                al, bl = need(runs)
                ao, bo = 997 + 41 * p + 13 * rot, 5003 + 29 * p + 7 * rot
                ao = (0, P - al, ao, ao)[p]
                bo = (bo, bo, 0, P - bl)[p]
                specs.append((ao, al, bo, bl, runs, bool(strand & 1), bool(strand & 2)))
    return specs


def strand_cells(specs, pool_len=len(POOL)):
    hit = set()
    ps = paths([len(s[4]) for s in specs])
    for q0 in range(0, len(specs), 4):
        quad = specs[q0:q0 + 4]
        if ps[q0] != "group":
            continue
        hit.add(("quad_strands", tuple(int(s[5]) | int(s[6]) << 1 for s in quad)))
        for ao, al, bo, bl, runs, a_rc, b_rc in quad:
            strand = int(a_rc) | int(b_rc) << 1
            if 17 <= len(runs) <= 32:
                hit.add(("row_17_32", strand))
            for side, off, ln, rc in (("a", ao, al, a_rc), ("b", bo, bl, b_rc)):
                if ln < 8:
                    hit.add(("narrow_side", side, ln))
                if 0 < ln < 8:
                    hit.add(("narrow_side_strand", side, rc))
                if ln and off == 0:
                    hit.add(("at_byte_0", side, rc))
                if ln and off + ln == pool_len:
                    hit.add(("at_last_byte", side, rc))
    return hit


STRAND_WANT = ({("quad_strands", tuple((p + rot) % 4 for p in range(4))) for rot in range(4)} |
               {("row_17_32", s) for s in range(4)} |
               {("narrow_side", side, n) for side in "ab" for n in range(8)} |
               {("narrow_side_strand", side, rc) for side in "ab" for rc in (False, True)} |
               {(where, side, rc) for where in ("at_byte_0", "at_last_byte") for side in "ab" for rc in (False, True)})


# ---- 3. a refused alignment beside good ones -----------------------------------------------------------------------------------------
CAUSES = ("op 3", "run longer than both sequences", "a past its end", "b past its end")


def make_bad(case, cause, at):
    """`case` with its run `at` made the first that the kernels refuse, for `cause`."""
    a, b, runs = case
    runs = list(runs)
    l = max(runs[at][1], 2)
    pa, pb = need(runs[:at])
    if cause == "op 3":
        runs[at] = (3, l)
    elif cause == "run longer than both sequences":
        runs[at] = (M, max(len(a), len(b)) + 1)
    elif cause == "a past its end":  # (a D run: b is not touched)
        runs[at] = (D, l)
        a = a[:pa + l - 1]
    else:
        assert cause == "b past its end"
        runs[at] = (I, l)
        b = b[:pb + l - 1]
    return a, b, runs


def refusal_batches():
    """(batch, index of the bad alignment, cause, run) -- a good quad, then the quad with one of its rows made bad."""
    good = [row(c, 130 + p) for p, c in enumerate((21, 32, 24, 28))]
    lead = [row(c, 134 + p) for p, c in enumerate((17, 3, 32, 22))]
    out = []
    for cause in CAUSES:
        for at in (5, 20):
            for pos in range(4):
                out.append((lead + good[:pos] + [make_bad(good[pos], cause, at)] + good[pos + 1:], 4 + pos, cause, at))
    for cause in CAUSES:  # once outside the grouped path: a 40-run alignment sends the quad to wavefronts of their own
        batch = [row(40, 138, (1, 2, 3, 4, 5)), make_bad(good[0], cause, 20), good[1], good[2]]
        out.append((batch, 1, cause, 20))
    return out


# ---- 4. whole alignments and segments ---------------------------------------------------------------------------------------------------
def _chunk64(units):
    """The lengths of 64 runs that make `units` units."""
    lens = {63: [8] * 63 + [0], 64: [7] * 64, 65: [1] * 63 + [9], 127: [9] * 63 + [1], 128: [16] * 64, 129: [15] * 63 + [17],
            191: [17] * 63 + [9], 192: [24] * 64, 193: [23] * 63 + [25]}[units]
    assert len(lens) == 64 and sum(_units(l) for l in lens) == units
    return lens


def _whole_table():
    c = _chunk64
    short = (1, 2, 3, 4, 5, 6, 7, 8, 9)
    batch = [aln(_ops(c(63) + c(64), 0), 140),  # 128 runs, a zero-length run at 63
             aln(_ops(c(65) + c(127) + [5], 1), 141),  # 129
             aln(_ops(c(128) + c(129)[1:], 2), 142),  # 127
             aln(_ops(c(191) + [1], 3), 143),  # 65
             aln(_ops(c(192), 4), 144),  # 64
             aln(_ops(c(64)[1:], 0), 145),  # 63
             aln(_ops(c(193) + c(129), 1), 146),
             aln(_ops(c(64) + [0] + [4] * 5, 2), 147),  # a zero-length run at 64
             row(33, 148), row(1, 149), row(0, 150), row(17, 151),  # (short ones in a quad that is not grouped)
             row(1023, 152, short), row(1024, 153, short)]
    want = {("whole_runs", n) for n in WHOLE_COUNTS + (0, 1, 17)} | {("whole_chunk_units", u) for u in WHOLE_UNITS}
    want |= {("whole_zero_at", 63), ("whole_zero_at", 64)}
    return Table("whole alignments", [batch], {GROUP_MAX: want})


WHOLE_TABLE = _whole_table()


def segment_runs(n_runs):
    """Runs of 0..5 columns, a zero-length one at some segment seams; the second segment consumes nothing of a, the third (1536, 1537 runs) nothing of b."""
    runs = []
    for k in range(n_runs):
        op = (M, D, M, I, M, M)[k % 6]
        if SEG <= k < 2 * SEG:
            op = I
        elif 2 * SEG <= k < 3 * SEG and n_runs >= 3 * SEG:
            op = D
        runs.append((op, 0 if k % SEG in (0, SEG - 1) and k % 3 == 0 else 1 + (7 * k) % 5))
    return runs


def segment_specs():
    """Per run count the four strand combinations: a ends at the pool's last byte, b starts at its byte 0."""
    P, specs = len(POOL), []
    for n_runs in SEGMENT_COUNTS:
        runs = segment_runs(n_runs)
        na, nb = need(runs)
        for strand in range(4):
            specs.append((P - na - 2, na + 2, 0, nb + strand, runs, bool(strand & 1), bool(strand & 2)))
    return specs


SEGMENT_WANT = {("segments_runs", n) for n in SEGMENT_COUNTS} | {"segment_without_a", "segment_without_b"}


def segment_count(n_runs):
    return (n_runs + SEG - 1) // SEG


def all_good_cases():
    """Every case of every table that is meant to fit its sequences."""
    out = [c for t in GROUP_TABLES + [WHOLE_TABLE] for b in t.batches for c in b]
    out += as_cases(strand_specs()) + as_cases(segment_specs())
    for batch, bad, _, _ in refusal_batches():
        out += batch[:bad] + batch[bad + 1:]
    return out
