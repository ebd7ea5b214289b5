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
