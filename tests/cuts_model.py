"""The piece records of sdf_stats_cuts_pairs on column strings, walked one column at a time like the host does
(csrc/host/stats.cc: split_alignment / subhit; csrc/host/alignment.cc: trim_back / trim_front), and their comparison with
the column-string model of tests/test_stats_generate.py (ColAln, _subhit, _split_alignment).  Shared by
tests/test_stats_cuts_cpu.py (where it is the CPU stand-in behind the host's hook) and tests/test_gpu_stats_cuts.py."""
import ctypes as C

import numpy as np

DEFAULT = (5, -4, -40, -1)  # match, mismatch, gap_open, gap_extend (Params, csrc/host/sedef_host.h)
OPS = "MDI"  # run words are len << 4 | op: 0 'M', 1 'D' (a only), 2 'I' (b only)


def _up(c):
    return c - 32 if 97 <= c <= 122 else c


def columns(a, b, runs):
    """a, b: bytes; runs: (op, len) with op 0 / 1 / 2.  Per column: kind (0 pair, 1 gap in b, 2 gap in a), N on a, N on b, match."""
    kind, na, nb, mt, ia, ib = [], [], [], [], 0, 0
    for op, n in runs:
        for _ in range(n):
            ca = _up(a[ia]) if op != 2 else None
            cb = _up(b[ib]) if op != 1 else None
            ia += op != 2
            ib += op != 1
            kind.append(op)
            na.append(ca == 78)
            nb.append(cb == 78)
            mt.append(op == 0 and ca == cb and ca != 78)
    return kind, na, nb, mt


def _trim(kind, mt, b, e, scores):
    ma, mm, go, ge = scores

    def scan(order):
        prev, score, seen = -1, 0, 0
        for i in order:
            k = kind[i]
            score += (ma if mt[i] else mm) if k == 0 else (go if prev != k else 0) + ge
            prev = k
            seen += mt[i]
            yield i, score, seen

    best, col, m = 0, -1, 0
    for i, score, seen in scan(range(b, e)):  # trim_back: the best prefix, ties to the longer
        if score >= best:
            best, col, m = score, i, seen
    if col < 0:
        return b, b, 0
    te = col + 1
    none = sum(1 for i in range(b, te) if kind[i] != 2)  # the reference's marker: the a-bases of what trim_back kept
    best, col, m = 0, none, 0
    for i, score, seen in scan(range(te - 1, b - 1, -1)):  # trim_front: the best suffix, ties to the longer
        if score >= best:
            best, col, m = score, i - b, seen
    if col == none:
        return b, b, 0
    return b + col, te, m


def records(a, b, runs, scores=DEFAULT):
    """[(begin, end, t_begin, t_end, matches)] of one alignment."""
    kind, na, nb, mt = columns(a, b, runs)
    span = len(kind)
    cut, prev, begin = [], [0, 0], 0
    for i in range(span):
        for side, isn in enumerate((na[i], nb[i])):
            if isn:
                prev[side] += 1
            else:
                if prev[side] >= 100:
                    if i - prev[side] > begin:
                        cut.append((begin, i - prev[side]))
                    begin = i
                prev[side] = 0
    if not begin:
        return [(0, span, 0, span, sum(mt))]
    if begin < span:
        cut.append((begin, span))
    return [(s, e) + _trim(kind, mt, s, e, scores) for s, e in cut]


def hook(calls=None):
    """A CUTS_HOOK (sedef_amd.host) that answers with records(); calls: a list that receives (a, b, runs, records)."""
    from sedef_amd.host import CUTS_HOOK

    def fn(a, a_len, b, b_len, runs, n_runs, scores, out, cap):
        sa, sb = C.string_at(a, a_len), C.string_at(b, b_len)
        rr = [(int(runs[k]) & 15, int(runs[k]) >> 4) for k in range(n_runs)]
        recs = records(sa, sb, rr, tuple(int(scores[k]) for k in range(4)))
        if calls is not None:
            calls.append((sa, sb, rr, recs))
        for k, r in enumerate(recs[:cap]):
            for f in range(5):
                out[8 * k + f] = r[f]
            out[8 * k + 5] = out[8 * k + 6] = out[8 * k + 7] = 0
        return len(recs)
    return CUTS_HOOK(fn)


def check_against_column_model(a, b, runs, recs):
    """The pieces the records describe are the pieces _split_alignment of tests/test_stats_generate.py cuts (default scores)."""
    from test_stats_generate import ColAln, _cigar_from_columns, _split_alignment
    sa, sb = a.decode("latin-1"), b.decode("latin-1")
    ops = [(OPS[op], n) for op, n in runs if n]
    h = dict(aln=ColAln(sa, sb, ops), qs=0, qe=len(sa), rs=0, re=len(sb), rc=False)
    exp = _split_alignment(h, -1, 1000)
    assert len(exp) == len(recs), (len(exp), recs)
    ca, cb = ColAln(sa, sb, ops).columns()
    if len(recs) == 1 and recs[0][0] == 0:  # no event: the alignment as it is
        assert exp[0]["aln"] is h["aln"] and recs[0][:4] == (0, len(ca), 0, len(ca)) and recs[0][4] == h["aln"].counters()[3]
        return
    for (s, e, ts, te, m), p in zip(recs, exp):
        assert (p["qs"], p["qe"]) == (len(ca[:s].replace("-", "")), len(ca[:e].replace("-", ""))), (s, e)
        assert (p["rs"], p["re"]) == (len(cb[:s].replace("-", "")), len(cb[:e].replace("-", ""))), (s, e)
        al = p["aln"]
        assert (al.a, al.b) == (ca[ts:te].replace("-", ""), cb[ts:te].replace("-", "")), (s, e, ts, te)
        assert al.cigar == (_cigar_from_columns(ca[ts:te], cb[ts:te]) if te > ts else []), (s, e, ts, te)
        assert m == (al.counters()[3] if te > ts else 0)


# ---- hand-made alignments: (name, a, b, runs) on the strings as the alignment reads them --------------------------------
def make(rng, runs, n_a=(), n_b=(), sub=0.03, force=None):
    """Random bases under `runs`; b copies a on pair columns (substitutions at rate `sub`); n_a / n_b: column ranges whose
    bases of that side become N; force: {column: 'match' | 'mismatch'} on pair columns."""
    alpha = np.frombuffer(b"ACGT", np.uint8)
    a, b, col_a, col_b, ia, ib = [], [], [], [], 0, 0
    for op, n in runs:
        for _ in range(n):
            c = len(col_a)
            x = int(alpha[rng.integers(0, 4)])
            if op == 0:
                y = x
                want = (force or {}).get(c)
                if want == "mismatch" or (want is None and rng.random() < sub):
                    y = int(alpha[(list(alpha).index(x) + 1 + rng.integers(0, 3)) % 4])
                a.append(x), b.append(y)
            elif op == 1:
                a.append(x)
            else:
                b.append(x)
            col_a.append(ia if op != 2 else -1)
            col_b.append(ib if op != 1 else -1)
            ia += op != 2
            ib += op != 1
    a, b = np.array(a, np.uint8), np.array(b, np.uint8)
    for side, cols, rngs in ((a, col_a, n_a), (b, col_b, n_b)):
        for s, e in rngs:
            for c in range(s, e):
                if cols[c] >= 0:
                    side[cols[c]] = 78
    low = rng.random(len(a)) < 0.2
    a = np.where(low & (a != 78), a | 0x20, a).astype(np.uint8)
    return a.tobytes(), b.tobytes(), [(op, n) for op, n in runs]


def handmade(rng):
    M, D, I = 0, 1, 2
    cases = []

    def add(name, *args, **kw):
        cases.append((name,) + make(rng, *args, **kw))

    for L in (99, 100, 101):  # run lengths, in a, in b, in both ending at the same column (a's event first)
        add("a%d" % L, [(M, 400)], n_a=[(150, 150 + L)])
        add("b%d" % L, [(M, 400)], n_b=[(150, 150 + L)])
        add("ab%d" % L, [(M, 400)], n_a=[(250 - L, 250)], n_b=[(130, 250)])
        add("ba%d" % L, [(M, 400)], n_b=[(250 - L, 250)], n_a=[(130, 250)])
    add("run to the last column", [(M, 400)], n_a=[(280, 400)])
    add("run from column 0", [(M, 400)], n_b=[(0, 120)])
    add("run from column 0 and to the last", [(M, 400)], n_a=[(0, 110)], n_b=[(290, 400)])
    add("overlapping runs", [(M, 400)], n_b=[(50, 200)], n_a=[(60, 180)])
    add("run broken by a gap", [(M, 160), (I, 1), (M, 240)], n_a=[(100, 221)])
    add("gap beside the run", [(M, 90), (I, 1), (M, 310)], n_a=[(100, 220)])
    add("piece starts inside a gap run", [(M, 195), (I, 20), (M, 200)], n_b=[(100, 205)])
    add("piece starts inside a D run", [(M, 195), (D, 20), (M, 200)], n_a=[(100, 205)])
    for lead in (5, 6):  # the trim_front marker: the best suffix starts at column 15 = the a-bases of the piece
        add("marker quirk, %d leading matches" % lead, [(M, lead), (I, 10), (M, 310)], n_a=[(lead + 20, lead + 120)],
            force={c: "match" for c in list(range(lead)) + list(range(lead + 10, lead + 20)) + list(range(lead + 120, lead + 310))})
    # (with a D run in the place of the I run the piece has 25 a-bases, the marker is not met and the last ten columns stay)
    add("marker not met", [(M, 5), (D, 10), (M, 310)], n_b=[(25, 125)],
        force={c: "match" for c in list(range(5)) + list(range(15, 25)) + list(range(125, 315))})
    add("piece of mismatches", [(M, 400)], n_a=[(20, 120)], force={c: "mismatch" for c in range(20)})
    tie = {c: "mismatch" for c in range(5)}
    tie.update({c: "match" for c in range(5, 9)})
    add("whole piece scores 0", [(M, 400)], n_b=[(9, 130)], force=tie)
    tie = {c: "match" for c in list(range(4)) + list(range(9, 13))}
    tie.update({c: "mismatch" for c in range(4, 9)})
    add("two suffixes of one score", [(M, 400)], n_b=[(13, 130)], force=tie)
    for before in (63, 64, 65, 127, 128, 129):  # an event and a piece boundary across a chunk of 64 runs
        head = [(M, 1), (D, 1)] * (before // 2) + ([(M, 1)] if before % 2 else [])
        last = head[-1][0]
        runs = head + [(I if last == M else M, 3)] + ([(M, 300)] if last == M else [(I, 2), (M, 300)])
        c0 = sum(n for _, n in runs[:-1])
        add("%d runs before the run" % before, runs, n_a=[(c0 + 20, c0 + 125)], n_b=[(c0 + 140, c0 + 245)])
    for k in range(9):  # ... across the unit of eight columns
        add("unit edge %d" % k, [(M, 37), (D, 2), (M, 400)], n_a=[(60 + k, 160 + 2 * k)], n_b=[(200 + k, 300 + k)])
    runs = [(M, 1), (I, 1), (M, 1), (D, 1)] * 280 + [(M, 420)]  # more than 1,024 runs, N runs across the run 1,024 / 1,088 marks
    add("1121 runs", runs, n_a=[(1120, 1240)], n_b=[(1300, 1420)])
    add("no event", [(M, 150), (D, 7), (M, 100), (I, 9), (M, 200)], n_a=[(40, 139)], n_b=[(300, 380)])
    return cases


# ---- the second model: whole arrays, from the definition at the head of csrc/stats_cuts.hip ------------------------------
def columns_np(a, b, runs):
    """columns() on arrays: kind (int8), N on a, N on b, match (bool), one entry per column."""
    r = np.asarray(runs, np.int64).reshape(-1, 2)
    kind = np.repeat(r[:, 0], r[:, 1]).astype(np.int8)
    out = []
    for s, absent in ((a, 2), (b, 1)):
        v = np.frombuffer(s, np.uint8)
        v = np.where((v >= 97) & (v <= 122), v - 32, v).astype(np.int16)
        have = kind != absent
        assert int(have.sum()) <= len(v), "the runs read past a sequence"
        c = np.full(len(kind), -1, np.int16)  # (-1: the side has no base in this column)
        c[have] = v[:int(have.sum())]
        out.append(c)
    ca, cb = out
    return kind, ca == 78, cb == 78, (kind == 0) & (ca == cb) & (ca != 78)


def _n_events(mask, side, span):
    """The events of one side: (e, side, s) for every maximal run [s, e) of the mask with e - s >= 100 and e < span."""
    edge = np.diff(np.concatenate(([0], mask.astype(np.int8), [0])))
    s, e = np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)
    keep = (e - s >= 100) & (e < span)
    return [(int(y), side, int(x)) for x, y in zip(s[keep], e[keep])]


def events_np(na, nb):
    """The events in order: by e, side a before side b."""
    return sorted(_n_events(na, 0, len(na)) + _n_events(nb, 1, len(nb)))


def scores_np(kind, mt, scores):
    """F (span + 1 entries: the sum of the columns' scores before column i) and G (span entries)."""
    ma, mm, go, ge = scores
    gap = kind != 0
    before = np.concatenate(([-1], kind[:-1])) if len(kind) else kind
    cont = gap & (before == kind)  # the column continues a gap in the same sequence
    c = np.where(gap, ge + np.where(cont, 0, go), np.where(mt, ma, mm)).astype(np.int64)
    F = np.concatenate(([0], np.cumsum(c)))
    return F, F[:-1] - go * cont


def trim_np(kind, mt, F, G, b, e):
    """trim_back, then trim_front, of columns [b, e): (t_begin, t_end, matches)."""
    if e <= b:
        return b, b, 0
    te = e - int(np.argmax(F[b + 1:e + 1][::-1]))  # behind the LAST argmax of F(i + 1)
    if F[te] - G[b] < 0:
        return b, b, 0
    tb = b + int(np.argmin(G[b:te]))  # the FIRST argmin of G
    if F[te] - G[tb] < 0 or tb - b == int((kind[b:te] != 2).sum()):
        return b, b, 0
    return tb, te, int(mt[tb:te].sum())


def records_np(a, b, runs, scores=DEFAULT):
    """records(), on arrays."""
    kind, na, nb, mt = columns_np(a, b, runs)
    span = len(kind)
    ev = events_np(na, nb)
    if not ev:
        return [(0, span, 0, span, int(mt.sum()))]
    e = np.array([x[0] for x in ev], np.int64)
    s = np.array([x[2] for x in ev], np.int64)
    begin = np.concatenate(([0], e[:-1]))  # what an event sees: the e of the event before it
    cut = [(int(x), int(y)) for x, y in zip(begin[s > begin], s[s > begin])] + [(int(e[-1]), span)]
    F, G = scores_np(kind, mt, scores)
    return [(x, y) + trim_np(kind, mt, F, G, x, y) for x, y in cut]


def make_np(rng, runs, n_a=(), n_b=(), sub=0.03, force=None):
    """make() on arrays (another draw of the bases); force: per column, > 0 a match, < 0 a mismatch, 0 as drawn.  Runs of
    length 0 stay in the list that is returned."""
    r = np.asarray(runs, np.int64).reshape(-1, 2)
    kind = np.repeat(r[:, 0], r[:, 1])
    span = len(kind)
    x = rng.integers(0, 4, span)
    miss = rng.random(span) < sub
    if force is not None:
        f = np.asarray(force)
        assert len(f) == span
        miss = np.where(f > 0, False, np.where(f < 0, True, miss))
    y = (x + np.where(miss, rng.integers(1, 4, span), 0)) % 4
    alpha = np.frombuffer(b"ACGT", np.uint8)
    out = []
    for idx, rngs, absent in ((x, n_a, 2), (y, n_b, 1)):
        c = alpha[idx].copy()
        for s, e in rngs:
            c[s:e] = 78
        low = (rng.random(span) < 0.2) & (c != 78)
        c[low] |= 0x20
        out.append(c[kind != absent].tobytes())
    return out[0], out[1], [(int(op), int(n)) for op, n in runs]


def random_cases(rng, n=300):
    """The random alignments of tests/test_gpu_stats_cuts.py::test_random_batch_and_other_scores (the same draws, so with
    default_rng(9) the same cases): (name, a, b, runs, a_rc, b_rc)."""
    out = []
    for k in range(n):
        runs, cols = [], 0
        while cols < 120 or (len(runs) < 3 and rng.random() < 0.7):
            op = 0 if not runs or runs[-1][0] != 0 else int(rng.integers(1, 3))
            ln = int(rng.integers(20, 260)) if op == 0 else int(rng.integers(1, 12))
            runs.append((op, ln))
            cols += ln
        if runs[-1][0] != 0:
            runs.append((0, int(rng.integers(5, 60))))
            cols += runs[-1][1]
        plant = lambda: [(s, s + int(rng.integers(90, 111))) for s in rng.integers(0, max(cols - 100, 1), int(rng.integers(0, 3)))]  # noqa: E731
        n_a = [(s, min(e, cols)) for s, e in plant()]
        n_b = [(s, min(e, cols)) for s, e in plant()]
        a, b, runs = make(rng, runs, n_a=n_a, n_b=n_b, sub=float(rng.choice([0.02, 0.3, 0.7])))
        out.append(("r%d" % k, a, b, runs, bool(rng.integers(0, 2)), bool(rng.integers(0, 2))))
    return out


# ---- what a case's geometry is, for the conditions the seam families set themselves --------------------------------------
def run_starts(runs):
    """The first column of every run (and the span behind the last)."""
    return np.concatenate(([0], np.cumsum([n for _, n in runs]))).astype(np.int64)


def unit_of(runs, col):
    """(run index, unit of eight columns inside the run, unit index in the alignment) of a column: the kernel's work items."""
    st = run_starts(runs)
    j = int(np.searchsorted(st, col, side="right")) - 1
    while runs[j][1] == 0:
        j += 1
    units = np.concatenate(([0], np.cumsum([(n + 7) // 8 for _, n in runs])))
    u = (col - int(st[j])) // 8
    return j, u, int(units[j]) + u


def round_of(runs, col):
    """(chunk of 64 runs, round of 64 units inside the chunk, lane) that holds the column."""
    j, u, _ = unit_of(runs, col)
    base = j - j % 64
    before = sum((n + 7) // 8 for _, n in runs[base:j])
    return j // 64, (before + u) // 64, (before + u) % 64


# ---- cases aimed at the seams of stats_cuts.hip: chunks of 64 runs, rounds of 64 units, tasks 1024 at a time --------------
M, D, I = 0, 1, 2
SEAM_SCORES = (DEFAULT, (0, 0, 0, 0), (1, -1, 0, 0), (63, -63, -32, -31))


class _Lay:
    """Runs laid one after the other (runs of one op merge), with the column where the next one starts."""

    def __init__(self):
        self.runs, self.col, self.n_a, self.n_b = [], 0, [], []

    def add(self, op, n):
        if self.runs and self.runs[-1][0] == op:
            self.runs[-1] = (op, self.runs[-1][1] + n)
        else:
            self.runs.append((op, n))
        self.col += n

    def run_start(self):
        return self.col - self.runs[-1][1]


def _many_pieces(rng, variant, events=150):
    """N runs of 100-110 columns with 20-40 bases between them and a short gap run in every stretch between."""
    lay, deltas, k = _Lay(), (-3, 0, 2, -1, 0, 3, 1, -2), 0
    lay.add(M, 25)
    made = 0
    while made < events:
        lay.add((D, I)[k % 2], 1 + k % 3)
        lay.add(M, int(rng.integers(8, 16)))
        r0 = lay.run_start()
        if variant == "a":
            s = lay.col
            e = s + int(rng.integers(100, 111))
            lay.n_a.append((s, e)), lay.add(M, e - s)
            made += 1
        elif variant == "alternating":
            s = lay.col
            e = s + int(rng.integers(100, 111))
            (lay.n_a, lay.n_b)[k % 2].append((s, e)), lay.add(M, e - s)
            made += 1
        elif variant == "one unit":  # both sides end inside one unit of eight columns: e_a - e_b = delta
            d = deltas[k % 8]
            lo = r0 + 8 * ((lay.col - r0 + 112) // 8 + 1) + 2  # the earlier end: column 2 of a unit of this run
            e_a, e_b = (lo, lo - d) if d <= 0 else (lo + d, lo)
            lay.n_a.append((e_a - int(rng.integers(100, 111)), e_a))
            lay.n_b.append((e_b - int(rng.integers(100, 111)), e_b))
            lay.add(M, max(e_a, e_b) - lay.col)
            made += 2
        else:  # "overlapping": side b's run begins inside side a's and ends behind it
            s = lay.col
            lay.n_a.append((s, s + 105)), lay.n_b.append((s + 50, s + 160)), lay.add(M, 160)
            made += 2
        lay.add(M, int(rng.integers(8, 16)))
        k += 1
    lay.add(M, 60)
    return lay


def seam_cases(rng):
    """[(family, name, a, b, runs)]: see the families in tests/test_stats_cuts_cpu.py, where each one's condition is checked."""
    cases = []

    def add(family, name, runs, **kw):
        cases.append((family, name) + make_np(rng, runs, **kw))

    # -- N runs that end or start around column 512 of one M run (unit 64: the first of the second round)
    for side in "ab":
        for L in (100, 99):
            for d in (-8, -1, 0, 1, 7, 8):
                add("round seam", "%s%d ends at 512%+d" % (side, L, d), [(M, 1100)], **{"n_" + side: [(512 + d - L, 512 + d)]})
        for s in (511, 512, 513):
            add("round seam", "%s starts at %d" % (side, s), [(M, 1100)], **{"n_" + side: [(s, s + 100)]})
    # -- N runs across several rounds and chunks
    for side, other in ("ab", "ba"):
        add("long run", "700 on %s, 5000 on %s" % (side, other), [(M, 7000)], **{"n_" + side: [(200, 900)], "n_" + other: [(1500, 6500)]})
    for gap, name in ((D, "D"), (I, "I")):
        runs = [(M, 300)] + [(gap, 5), (M, 10)] * 199 + [(gap, 5), (M, 310)]
        for side in "ab":
            add("long run", "%s 3000 under 200 M10/%s5" % (side, name), runs, **{"n_" + side: [(300, 3300)]})
    # -- more pieces than lanes
    for variant in ("a", "alternating", "one unit", "overlapping"):
        lay = _many_pieces(rng, variant)
        add("many pieces", variant, lay.runs, n_a=lay.n_a, n_b=lay.n_b)
    # -- piece begins and ends on every residue mod 8 and on units 63, 64, 65 of a round; pieces that begin inside gap runs
    n_a, n_b = [], []
    for k in range(8):
        (n_a, n_b)[k % 2].append((200 * k + 40 + k, 200 * k + 140 + k))
    for k, (r, off) in enumerate(((4, -5), (5, 3), (6, 11))):  # piece begins: units 63, 64 (the next round's first), 65
        (n_a, n_b)[k % 2].append((512 * r + off - 103, 512 * r + off))
    for k, (r, off) in enumerate(((7, -5), (8, 3), (9, 11))):  # piece ends
        (n_b, n_a)[k % 2].append((512 * r + off, 512 * r + off + 101))
    add("piece edges", "every residue", [(M, 5400)], n_a=n_a, n_b=n_b)
    add("piece edges", "begins inside an I run", [(M, 195), (I, 20), (M, 800)], n_b=[(100, 205)])
    add("piece edges", "begins inside a D run", [(M, 195), (D, 20), (M, 800)], n_a=[(100, 205)])
    for gap, other, side in ((I, D, "b"), (D, I, "a")):
        head = [(M, 3), (gap, 1)] * 31
        c0 = 4 * 31
        add("piece edges", "begins inside the %s run at index 63" % OPS[gap], head + [(M, 120), (gap, 20), (M, 700)],
            **{"n_" + side: [(c0 + 10, c0 + 125)]})
        add("piece edges", "begins inside the %s run at index 64" % OPS[gap], head + [(other, 1), (M, 120), (gap, 20), (M, 700)],
            **{"n_" + side: [(c0 + 11, c0 + 126)]})
    # -- 3,000 runs of 1-7 columns; three windows without the op that would break the planted run
    ops, lens, windows = [], rng.integers(1, 8, 3000), ((400, 470, I), (1300, 1370, D), (2400, 2470, I))
    for k in range(3000):
        banned = [w[2] for w in windows if w[0] <= k < w[1]]
        ops.append(int(rng.choice([o for o in (M, D, I) if o not in banned and (not ops or o != ops[-1])])))
    runs = [(o, int(n)) for o, n in zip(ops, lens)]
    st = run_starts(runs)
    plant = [(int(st[lo + 8]) + 3, int(st[lo + 8]) + 3 + 104 + 3 * i) for i, (lo, hi, _) in enumerate(windows)]
    assert all(e < int(st[hi - 8]) for (_, e), (lo, hi, _) in zip(plant, windows))
    add("short units", "3000 runs", runs, n_a=[plant[0], plant[2]], n_b=[plant[1]])
    # -- runs of length 0
    base = [(M, 5), (D, 1)] * 40 + [(M, 600)]
    for at, name in ((63, "at index 63"), (64, "at index 64"), (0, "first"), (len(base), "last")):
        for op in (M, I):
            add("zero runs", "%s 0 %s" % (OPS[op], name), base[:at] + [(op, 0)] + base[at:], n_a=[(130, 240)], n_b=[(500, 610)])
    for second, tail, name in ((D, 10, "D 3, M 0, D 4"), (I, 12, "D 3, M 0, I 4")):
        runs = [(M, 200), (D, 3), (M, 0), (second, 4), (M, tail + 400)]
        force = np.zeros(607 + tail, np.int8)
        force[150:207 + tail] = 1  # what follows the gaps up to the N run: matches
        add("zero runs", name, runs, n_b=[(207 + tail, 307 + tail)], force=force)
    # -- trims whose extremes tie far apart, across lanes and rounds ((1, -1, 0, 0); with (0, 0, 0, 0) every case ties)
    force = -np.ones(2400, np.int8)
    force[100:600] = force[1100:1600] = 1
    force[2100:] = 0
    add("trim ties", "two maxima, two minima", [(M, 2400)], n_a=[(2000, 2100)], force=force)
    force = -np.ones(1100, np.int8)
    force[:512] = 1
    force[800:] = 0
    add("trim ties", "maximum on both sides of a round", [(M, 512), (D, 3), (M, 585)], n_a=[(700, 800)], force=force)
    force = -np.ones(4700, np.int8)
    force[2000:4100] = force[4200:4250] = 1
    add("trim ties", "deep F", [(M, 4700)], n_b=[(4100, 4200)], force=force)
    add("trim ties", "piece of I columns", [(M, 150), (I, 400), (M, 150)], n_b=[(20, 170), (250, 400)])
    add("trim ties", "piece of D columns", [(M, 150), (D, 400), (M, 150)], n_a=[(20, 170), (250, 400)])
    # -- a side shorter than eight bases
    for short, head, tail in ((0, 0, 0), (3, 2, 1), (7, 3, 4)):
        for gap, side in ((I, "b"), (D, "a")):
            runs = [r for r in ((M, head), (gap, 310 + short), (M, tail)) if r[1]]
            add("narrow", "%d bases beside %s" % (short, OPS[gap]), runs, **{"n_" + side: [(head + 50, head + 160)]})
    # -- a piece over the chunk seam, where the chunk's last run (index 63) opens a gap and its last round has idle lanes
    force = np.zeros(752, np.int8)
    force[320:500] = 1
    add("piece edges", "over a chunk that ends with an opening gap", [(M, 9), (D, 1)] * 31 + [(M, 140), (I, 2), (M, 300)],
        n_a=[(200, 320)], n_b=[(500, 610)], force=force)
    return cases


def real_size_case(rng):
    """200,000 columns, about 400 runs; a 50,000-column N run on side a (under M and D runs only) and one of 120 on side b."""
    lay, k = _Lay(), 0
    while lay.col < 198000:
        lay.add(M, int(rng.integers(300, 1500)))
        inside = 60000 <= lay.col < 113000
        lay.add(D if inside or k % 2 else I, int(rng.integers(1, 40)))
        k += 1
    lay.add(M, 200000 - lay.col)
    st = run_starts(lay.runs)
    j = int(np.searchsorted(st, 150000))  # the first M run that starts behind column 150,000 holds b's N run
    j += lay.runs[j][0] != M
    return ("real size", "200,000 columns") + make_np(rng, lay.runs, n_a=[(61000, 111000)], n_b=[(int(st[j]) + 90, int(st[j]) + 210)], sub=0.05)


def small_cases(rng, n):
    """n alignments of 130-300 columns, 3-5 runs, 0-2 events: the batch that crosses the scan kernel's blocks of 1,024."""
    out = []
    for k in range(n):
        span = int(rng.integers(130, 301))
        gap, g, g2, c0 = int(rng.integers(1, 3)), int(rng.integers(1, 6)), int(rng.integers(1, 6)), int(rng.integers(10, span - 60))
        if k % 3:
            m2 = int(rng.integers(5, span - c0 - g - g2 - 10))
            runs = [(M, c0), (gap, g), (M, m2), (3 - gap, g2), (M, span - c0 - g - m2 - g2)]
        else:
            runs = [(M, c0), (gap, g), (M, span - c0 - g)]
        total = sum(x for _, x in runs)
        ev = int(rng.integers(0, 3))
        rngs = [(s, min(s + int(rng.integers(95, 111)), total)) for s in rng.integers(0, max(total - 105, 1), ev)]
        if ev == 2 and k % 4 == 0 and span >= 250:  # three pieces: both runs whole, one behind the other, the gap run behind them
            runs = [(M, span - g - 12), (gap, g), (M, 12)]
            rngs = [(6, 106 + k % 5), (116 + k % 7, 218 + k % 7)]
        out.append(("batch", "s%d" % k) + make_np(rng, runs, n_a=rngs[:1], n_b=rngs[1:], sub=0.1))
    return out
