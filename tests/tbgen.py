"""Designed CIGARs for the traceback tests (tests/test_tbgen_cpu.py, tests/test_gpu_traceback.py): plain numpy, no GPU.

sedef_amd/csrc/traceback.hip walks a task a RUN at a time: a group of G lanes (16 or 64) covers at most G cells of a run per
round, then the run pauses and the next round continues it.  The inputs here put runs -- diagonal runs, E / F gap runs, runs
that end at the matrix edge -- at G - 1, G, G + 1, 2G, 2G + 1 cells, which random mutation (single-base indels) never does.

A designed case is `head + tail` against `head + gap + tail` with gap[0] != tail[0] and gap[-1] != head[-1]: under SEDEF's
scoring (5, -4, 40, 1) every other placement of the gap costs a mismatch, so the CPU oracle's CIGAR is exactly
[len(head) M, len(gap) D or I, len(tail) M].  The EXPECTED CIGAR of a test is always the oracle's; the design (`Case.runs`)
is a separate assertion on the oracle's output (tests/test_tbgen_cpu.py: no case may miss it).  ksw ops: 0 M, 1 I (consumes the
query), 2 D (consumes the target).

`ROUTES` names, per direction-flag layout, the settings that force the DP kernel writing it (those of
tests/test_gpu_fuzz_slice.py) and `route_cases` the smallest shapes that route accepts."""
import numpy as np

M, INS, DEL = 0, 1, 2
REV_CIGAR, EXTZ_ONLY, SCORE_ONLY = 0x80, 0x40, 0x01
GROUPS = (16, 64)


class Case:
    __slots__ = ("q", "t", "w", "zdrop", "flag", "runs", "family", "tag")

    def __init__(self, q, t, w, runs, family, tag, zdrop=-1, flag=0):
        self.q, self.t = np.ascontiguousarray(q, np.uint8), np.ascontiguousarray(t, np.uint8)
        self.w, self.zdrop, self.flag = int(w), int(zdrop), int(flag)
        self.runs = None if runs is None else [(int(op), int(ln)) for op, ln in runs if ln > 0]  # designed (op, len) list
        self.family, self.tag = family, tag

    def designed_words(self):
        return [(ln << 4) | op for op, ln in self.runs]


def edge_lengths(G):
    """Run lengths around the group size: a run of G cells ends a round exactly, G + 1 pauses once, 2G + 1 twice."""
    return [G - 1, G, G + 1, 2 * G - 1, 2 * G, 2 * G + 1, 3 * G + 5]


def edge_flanks(G):
    return [G - 1, G, G + 1, 2 * G, 2 * G + 1]


def _bases(rng, n):
    return rng.integers(0, 4, n).astype(np.uint8)


def _norepeat(rng, n):
    """Bases of which no two neighbours are equal: shifted by one against itself such a block has no match at all."""
    return (np.cumsum(rng.integers(1, 4, n)) & 3).astype(np.uint8)


def _other(rng, b):
    return np.uint8((int(b) + int(rng.integers(1, 4))) & 3)


def interior(rng, head, L, tail, side, w, family=1, flag=0, tag=""):
    """head + tail against head + gap + tail; side DEL: the target carries the gap, INS: the query does."""
    h, g, tl = _bases(rng, head), _bases(rng, L), _bases(rng, tail)
    if tail and g[0] == tl[0]:
        g[0] = _other(rng, tl[0])
    if head and g[-1] == h[-1]:
        g[-1] = _other(rng, h[-1])
        if L == 1 and tail and g[0] == tl[0]:  # one base, two conditions: the third base differs from both
            g[0] = np.uint8(({0, 1, 2, 3} - {int(tl[0]), int(h[-1])}).pop())
    short, long_ = np.concatenate([h, tl]), np.concatenate([h, g, tl])
    q, t = (short, long_) if side == DEL else (long_, short)
    return Case(q, t, w, [(M, head), (side, L), (M, tail)], family,
                "f%d %s head %d L %d tail %d w %d%s" % (family, "DI"[side == INS], head, L, tail, w, tag), flag=flag)


def family1(rng, G, Ls=None, heads=None, tail_of=None, bands=("full", "wide")):
    """Interior gap: L and flanks at the edges of G, both sides, full band and w = L + 8."""
    out = []
    for L in (Ls or edge_lengths(G)):
        for head in (heads or edge_flanks(G)):
            for side in (DEL, INS):
                for b in bands:
                    w = {"full": -1, "wide": L + 8, "hug": L, "leave": L - 4}[b] if isinstance(b, str) else int(b)
                    tail = head + 3 if tail_of is None else tail_of(head)
                    out.append(interior(rng, head, L, tail, side, w, family=2 if b in ("hug", "leave") else 1))
    return out


def family2(rng, G, **kw):
    """Band edge: the interior gap with w = L (the path hugs the band's edge) and w = L - 4 (it cannot stay inside: cells
    below / above the stored range are walked in a forced state, or the band runs out).  Not design-asserted."""
    out = family1(rng, G, bands=("hug", "leave"), **kw)
    for c in out:
        c.runs = None
    return out


def family3(rng, Ls=(15, 16, 17, 63, 64, 65), body=80, band=None):
    """Gap at the matrix edge: gap + body / body + gap against body.  The walk leaves the matrix inside a group (lanes beyond
    the edge are not valid) and the leading gap is the residual push.  Leading form: [L D or I, body M]; the trailing form's
    shape varies (oracle-compared only)."""
    out = []
    for L in Ls:
        for side in (DEL, INS):
            w = -1 if band is None else L + band
            b, g = _bases(rng, body), _bases(rng, L)
            if g[-1] == b[0]:
                g[-1] = _other(rng, b[0])  # (else the gap could as well end one base earlier)
            if g[0] == b[0]:
                g[0] = _other(rng, b[0])
                if L == 1:
                    g[0] = _other(rng, b[0])
            lead, plain = np.concatenate([g, b]), b
            q, t = (plain, lead) if side == DEL else (lead, plain)
            out.append(Case(q, t, w, [(side, L), (M, body)], 3, "f3 lead %s L %d w %d" % ("DI"[side == INS], L, w)))
            g2 = _bases(rng, L)
            trail = np.concatenate([b, g2])
            q, t = (plain, trail) if side == DEL else (trail, plain)
            out.append(Case(q, t, w, None, 3, "f3 trail %s L %d w %d" % ("DI"[side == INS], L, w)))
    return out


def family4(rng, G, w=-1, lengths=None):
    """Pure diagonal to the origin: equal sequences, and sequences that differ by mismatches only (every fifth base)."""
    out = []
    for n in (lengths or edge_flanks(G)):
        a = _bases(rng, n)
        out.append(Case(a, a.copy(), w, [(M, n)], 4, "f4 equal %d w %d" % (n, w)))
        b = a.copy()
        for k in range(2, n, 5):
            b[k] = (b[k] + 1 + (k % 3)) & 3
        out.append(Case(a, b, w, [(M, n)], 4, "f4 mismatches %d w %d" % (n, w)))
    return out


def many_runs(rng, words, flag=0, w=-1, block=20):
    """M blocks of `block` bases with one-base gaps between them, alternately D and I, until the CIGAR has `words` words
    (odd: it starts and ends with an M block)."""
    assert words % 2 == 1
    q, t, runs = [], [], []
    # (blocks without equal neighbours: a D and an I a block apart could otherwise be traded, now and then, for that block
    # shifted by one base -- 11 chance matches of 20 are enough)
    prev = _norepeat(rng, block)
    for k in range(words // 2 + 1):
        blk = _norepeat(rng, block) if k else prev
        if k:
            side = DEL if k % 2 else INS
            g = _bases(rng, 1)
            # one base that differs from both of its neighbours: no other placement of the gap scores as much
            g[0] = np.uint8(min({0, 1, 2, 3} - {int(blk[0]), int(prev[-1])}))
            (t if side == DEL else q).append(g)
            runs.append((side, 1))
        q.append(blk)
        t.append(blk)
        runs.append((M, block))
        prev = blk
    return Case(np.concatenate(q), np.concatenate(t), w, runs, 5, "f5 %d words flag 0x%x w %d" % (words, flag, w), flag=flag)


def family5(rng, w=-1, counts=(63, 65, 129, 131), flags=(0, REV_CIGAR)):
    """Many runs: CIGARs of 63, 65 (one over the compaction's 64 words a pass), 129 and 131 words, forward and reversed
    (KSW_EZ_REV_CIGAR).  64 words: family5_even."""
    return [many_runs(rng, n, flag=f, w=w) for n in counts for f in flags]


def family5_even(rng, words=64, flag=0, w=-1):
    """An even number of words: a leading one-base deletion in front of words - 1 alternating words.  The leading gap's
    place is the oracle's business (not design-asserted)."""
    c = many_runs(rng, words - 1, flag=flag, w=w)
    g = np.array([_other(rng, c.t[0])], np.uint8)
    return Case(c.q, np.concatenate([g, c.t]), w, None, 5, "f5 %d words flag 0x%x w %d" % (words, flag, w), flag=flag)


def family6_general(rng):
    """Max-cell start on the general kernel: KSW_EZ_EXTZ_ONLY and z-drop 30 / 200; the sequences share their first part and
    go on with unrelated bases, so the walk starts inside the matrix; a leading gap makes it end with a residual push."""
    out = []
    for common in (63, 64, 65, 130):
        for lead in (0, 17):
            for zdrop, flag in ((30, 0), (200, 0), (-1, EXTZ_ONLY), (30, EXTZ_ONLY)):
                c = _bases(rng, common)
                g = _bases(rng, lead)
                if lead and g[-1] == c[0]:
                    g[-1] = _other(rng, c[0])
                q = np.concatenate([c, _bases(rng, 40)])
                t = np.concatenate([g, c, _bases(rng, 90)])
                out.append(Case(q, t, -1, None, 6, "f6 common %d lead %d zdrop %d flag 0x%x" % (common, lead, zdrop, flag),
                                zdrop=zdrop, flag=flag))
    return out


def family6_track(rng, bands=(15, 33, 64)):
    """Max-cell start on the default routing: banded tasks whose band runs out (|qlen - tlen| > w; the pair kernel's TRACK
    flavour, as tests/test_gpu_extz2.py: test_pair_kernel_track_band_runs_out)."""
    out = []
    for w in bands:
        for common in (63, 64, 65, 129, 200):
            for lead in (0, 9):
                c = _bases(rng, common)
                g = _bases(rng, lead)
                if lead and g[-1] == c[0]:
                    g[-1] = _other(rng, c[0])
                t = np.concatenate([g, c, _bases(rng, w + 40)])
                out.append(Case(c, t, w, None, 6, "f6 track common %d lead %d w %d" % (common, lead, w)))
    return out


# ---- routes: one per direction-flag layout (and per flavour that has a tb_addr branch or record form of its own) ----------
# settings: the library's configuration (sdf_config names); want: 7 every field (general kernel), 3 CIGAR + score
# (register-resident kernels); kinds: the TaskKind values (sedef_amd/csrc/sdf_internal.h) a planned task of the route has,
# nreg: its PlanTask::nreg where the route fixes it (None: any positive value; 0: the general kernel's byte rows)
K_GENERAL, K_GENERAL_HBM, K_PAIR, K_PLAIN, K_PLAIN_HBM, K_STRIPE, K_BSTRIPE, K_LANE, K_STRIP, K_CHAIN = 0, 1, 2, 3, 4, 5, 7, 8, 9, 10
ROUTES = {
    "general": dict(layout=0, settings=dict(SDF_FORCE_GENERAL=1), want=7, kinds=(K_GENERAL, K_PLAIN), nreg=0),
    "wave": dict(layout=1, settings=dict(SDF_NO_PAIR=1), want=3, kinds=(K_GENERAL,), nreg=None),
    "pair": dict(layout=2, settings=dict(), want=3, kinds=(K_PAIR,), nreg=None),
    "pair_mixed": dict(layout=2, settings=dict(SDF_MIXED_MIN=2), want=3, kinds=(K_PAIR,), nreg=None),
    "lane": dict(layout=5, settings=dict(SDF_LANE_MIN=1), want=3, kinds=(K_LANE,), nreg=None),
}
for _n in (1, 2, 4):
    ROUTES["stripe%d" % _n] = dict(layout=3, settings=dict(SDF_NO_STRIP=1, SDF_STRIPE_MIN=128, SDF_STRIPE_NREG=_n), want=3,
                                   kinds=(K_STRIPE,), nreg=_n)
    # (SDF_NO_MIXED: in a call of thousands of tasks the planner would move those whose band reaches the end to mixed pairs)
    ROUTES["bstripe%d" % _n] = dict(layout=4, settings=dict(SDF_BSTRIPE_MIN_ROWS=100, SDF_BSTRIPE_ALL=1, SDF_BSTRIPE_NREG=_n,
                                                            SDF_NO_MIXED=1), want=3, kinds=(K_BSTRIPE,), nreg=_n)
for _n in (4, 8):
    ROUTES["strip%d" % _n] = dict(layout=6, settings=dict(SDF_STRIP_ALWAYS=1, SDF_STRIP_COLS=_n), want=3,
                                  kinds=(K_STRIP, K_CHAIN), nreg=None)  # (nreg: 8 on the strip kernel, _n on a chain)


# the (route, G) calls of the GPU tests
CALLS = [(r, G) for r in sorted(ROUTES) for G in GROUPS if not (r == "lane" and G == 64) and not (r == "pair_mixed" and G == 16)]


def layout_of(kind, nreg):
    """dir_layout of sedef_amd/csrc/sdf_internal.h."""
    if nreg == 0:
        return 0
    return {K_PAIR: 2, K_STRIPE: 3, K_BSTRIPE: 4, K_LANE: 5, K_STRIP: 6, K_CHAIN: 6}.get(kind, 1)


def _seam_cases(rng, G, seam, bands, Ls=None):
    """Interior gaps around column `seam` of the target (a stripe seam, a strip's block edge): the gap starts one base
    before it, on it, one behind it, and lies across it; short tails at the edges of G (the walk's first run)."""
    out = []
    for L in (Ls or edge_lengths(G)):
        for k, head in enumerate((seam - 1, seam, seam + 1, seam - L // 2)):
            tail = (G + 4, 2 * G + 4)[k & 1]
            for side in (DEL, INS):
                for b in bands:
                    w = {"full": -1, "wide": L + 8, "hug": L, "leave": L - 4}[b]
                    c = interior(rng, head, L, tail, side, w, family=1 if b in ("full", "wide") else 2, tag=" seam %d" % seam)
                    if c.family == 2:
                        c.runs = None
                    out.append(c)
    return out


def route_cases(route, G, seed=20260):
    """The families in the smallest shapes `route` accepts, for walks in groups of G lanes."""
    rng = np.random.default_rng(seed + 97 * G + sum(map(ord, route)))
    if route == "general":
        return (family1(rng, G) + family2(rng, G) + family3(rng) + family3(rng, Ls=(15, 17, 64), band=8) + family4(rng, G) +
                family4(rng, G, w=7) + family5(rng) + [family5_even(rng, 64, f) for f in (0, REV_CIGAR)] + family6_general(rng))
    if route == "wave":  # banded tasks whose band reaches the end (a band that runs out goes to the general kernel here)
        return (family1(rng, G, bands=("wide",)) + family1(rng, G, bands=("hug",)) + family3(rng, band=8) + family4(rng, G, w=7) +
                family5(rng, w=16) + [family5_even(rng, 64, f, w=16) for f in (0, REV_CIGAR)])
    if route == "pair":  # ... and the TRACK flavour for those whose band runs out
        return (family1(rng, G, bands=("wide",)) + family2(rng, G) + family3(rng, band=8) + family4(rng, G, w=7) +
                family5(rng, w=16) + [family5_even(rng, 64, f, w=16) for f in (0, REV_CIGAR)] + family6_track(rng))
    if route == "pair_mixed":  # bands 64 / 128 that reach the end, lengths of 100 and more, no two tasks of one geometry
        # (G = 64 only: a mixed pair is two tasks WITHOUT a partner of their own geometry, and the planner forms such pairs
        # when they are at least a sixteenth of the chunk -- sdf_plan.hip, "keys.size() * 16 < cnt" -- which copies of a few
        # hundred cases never are)
        assert G == 64
        out = []
        for L in (15, 17, 33, 53, 63, 64, 65):
            out += family1(rng, G, Ls=[L], bands=(64 if L + 8 <= 64 else 128,))
        return out + [many_runs(rng, n, flag=f, w=64) for n in (65, 131) for f in (0, REV_CIGAR)]
    if route == "lane":  # both sequences of at most 256 bases, at most 16,384 cells, full band
        out = family1(rng, 16, bands=("full",))
        for L in (65, 129):
            out += [interior(rng, 20, L, 23, side, -1) for side in (DEL, INS)]
        return (out + family3(rng) + family4(rng, 16) + family4(rng, 64, lengths=(63, 64, 65, 127, 128)))
    if route.startswith("stripe"):  # full band, targets of 130..700 bases across the seam at 128 * nreg
        seam = 128 * int(route[6:])
        return _seam_cases(rng, G, seam, ("full",)) + family4(rng, G, lengths=(seam + G - 1, seam + G, seam + G + 1)) + \
            [many_runs(rng, n, flag=f) for n in (65, 131) for f in (0, REV_CIGAR) if seam < 512 or n == 65]
    if route.startswith("bstripe"):  # banded, 100 anti-diagonals and more; bands that hug the path and that run out
        seam = 128 * int(route[7:])
        return _seam_cases(rng, G, seam, ("wide", "hug", "leave")) + \
            family4(rng, G, w=7, lengths=(seam + G - 1, seam + G, seam + G + 1)) + \
            [many_runs(rng, n, flag=f, w=16) for n in (65, 131) for f in (0, REV_CIGAR) if seam < 512 or n == 65]
    if route.startswith("strip"):
        # full band; 257..512 target bases: one wavefront; 513..1,100: a chain, the gap across a block edge of 64 * cols
        # columns (256 or 512); an ODD number of cases in each form leaves one task without a partner
        out = _seam_cases(rng, G, 256, ("full",), Ls=edge_lengths(G)[:4])
        out += _seam_cases(rng, G, 512, ("full",), Ls=edge_lengths(G)[3:])
        out += family4(rng, G, lengths=(256 + G, 512 + G + 1)) + [many_runs(rng, n, flag=f) for n in (65, 131) for f in (0, REV_CIGAR)]
        # (a task of far more rows than any other: it pairs with its own copies only, and call_tasks makes their number odd)
        out.append(interior(rng, 300, 600, G + 4, INS, -1, tag=" odd one"))
        return out
    raise KeyError(route)


def pack(cases, copies=1, interleave_score_only=0):
    """(fields, pool): q_off, t_off, qlen, tlen, w, zdrop, flag as arrays, the cases `copies` times over (copy c of case k
    is task c * len(cases) + k; all copies name the same bytes of the pool)."""
    n = len(cases)
    off = np.zeros(2 * n + 1, np.int64)
    np.cumsum([len(s) for c in cases for s in (c.q, c.t)], out=off[1:])
    pool = np.concatenate([s for c in cases for s in (c.q, c.t)]) if n else np.zeros(0, np.uint8)
    f = dict(q_off=off[0:2 * n:2], t_off=off[1:2 * n:2], qlen=np.array([len(c.q) for c in cases], np.int32),
             tlen=np.array([len(c.t) for c in cases], np.int32), w=np.array([c.w for c in cases], np.int32),
             zdrop=np.array([c.zdrop for c in cases], np.int32), flag=np.array([c.flag for c in cases], np.int32))
    return {k: np.tile(v, copies) for k, v in f.items()}, pool


def tasks_of(cases, copies=1):
    """The same as a sedef_amd.TASK_DTYPE array."""
    from sedef_amd.extz2 import TASK_DTYPE
    f, pool = pack(cases, copies)
    t = np.zeros(len(cases) * copies, TASK_DTYPE)
    for k, v in f.items():
        t[k] = v
    return t, pool


def call_tasks(route, G):
    """(cases, copies, tasks, pool) of the one call that walks `route`'s cases in groups of G lanes: launch_chunk
    (sedef_amd/csrc/sdf_launch.hip: tb_solo) takes G = 64 for a one-chunk call of at most 8,192 tasks and G = 16 above, so
    the cases are there once (G = 64) or as many times over as it takes to pass 8,192 (G = 16).  The pair kernel wants a
    partner of the same geometry for every task (an even number of copies), a mixed pair two tasks of different
    geometry (an odd number), and the strip kernel's lone task an odd number of copies of the case nothing else pairs with."""
    cases = route_cases(route, G)
    copies = 8192 // len(cases) + 1 if G == 16 else 1
    if route == "pair":
        copies += copies & 1
    elif route == "pair_mixed" or route in ("strip4", "strip8"):
        copies += 1 - (copies & 1)
    assert (copies * len(cases) > 8192) == (G == 16)
    tasks, pool = tasks_of(cases, copies)
    return cases, copies, tasks, pool
