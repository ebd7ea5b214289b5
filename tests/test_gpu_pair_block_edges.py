"""The pair kernel (extz2_pair.hip) at the edges of its 16-row blocks and 32-row periods: the rows at which a block's
direction flags leave, the window re-bases, a row flavour hands over to the next one, the steady regime is entered, and a
mixed pair goes from its shared rows to one task in both halves.  Score, counters and every CIGAR word against the scalar
oracle; every call is planned first (sdf_debug_plan) and must be the pair kernel's with the expected number of window
registers, and the context must report the tasks as paired: no case can pass on another kernel.

The cases are chosen with the band schedule of the reference, lo0 = max(0, r - qlen + 1, (r - w + 1) >> 1), and with the
kernel's block predicate for the steady regime (extz2_pair.hip, "pure band regime on all 16 rows"), both written out below
ONLY to pick shapes and to assert that the shapes hit what their test names: what is computed is checked against the oracle
alone.  The shared rows of a mixed pair are pair_shared_rows / pair_clip_free of extz2_geom.h."""
import ctypes as C

import numpy as np
import pytest

from oracle.binding import mutate, random_codes
from util import cigar_to_str

pytestmark = pytest.mark.gpu

K_PAIR = 2  # TaskKind of sedef_amd/csrc/sdf_internal.h, as tests/tbgen.py
# most window registers of 64 slots a band takes (short targets: fewer): the planner needs ncol16 + 32 slots with
# ncol16 = ((min(qlen, tlen, w + 1) + 15) / 16 + 1) * 16, so 64 (one register) takes w <= 15
NREG_OF_BAND = {128: 3, 64: 2, 12: 1}
EDGE_ROWS = (15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65)
FIELDS = ("score", "mte", "mte_q", "zdropped")


def _plan(tasks, want):
    """per task: (chunk, launch class, nreg, kind, ., ., partner) -- the plan a context made now would run."""
    import sedef_amd
    from sedef_amd import extz2
    lib = sedef_amd.load_library()
    sc = extz2._scoring(extz2.sedef_mat(), 40, 1)
    n = len(tasks)
    per_task = np.zeros((n, 7), np.int64)
    per_chunk = np.zeros((64, 5), np.int64)
    nch = C.c_size_t(0)
    lib.sdf_debug_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_size_t, C.c_int, C.c_int, C.c_void_p,
                                   C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    rc = lib.sdf_debug_plan(C.byref(sc), tasks.ctypes.data, n, want, 64 << 30, 160 * 1024, 0, per_task.ctypes.data,
                            per_chunk.ctypes.data, 64, C.byref(nch))
    assert rc == 0
    return per_task


def _tasks_of(pairs, w):
    import sedef_amd
    tasks = np.zeros(len(pairs), sedef_amd.TASK_DTYPE)
    chunks, off = [], 0
    for k, (q, t) in enumerate(pairs):
        tasks["q_off"][k], tasks["qlen"][k] = off, len(q)
        off += len(q)
        tasks["t_off"][k], tasks["tlen"][k] = off, len(t)
        off += len(t)
        chunks += [q, t]
    tasks["w"], tasks["zdrop"] = w, -1
    return tasks, np.concatenate(chunks)


def _run(oracle, pairs, w, nreg, settings=None, mixed=False, solo_ok=0, full_window=True):
    """Plans and runs `pairs` at band w; every task but `solo_ok` of them must be planned to the pair kernel with a partner
    and at most `nreg` window registers (a target shorter than the band's window takes fewer) -- with full_window some with
    exactly `nreg` --, and the context must have run as many two to a wavefront."""
    import sedef_amd
    want = sedef_amd.extz2.WANT_CIGAR | sedef_amd.extz2.WANT_SCORE
    assert len(pairs) <= 400
    tasks, pool = _tasks_of(pairs, w)
    pt = _plan(tasks, want)
    me = np.arange(len(pt))
    paired = (pt[:, 3] == K_PAIR) & (pt[:, 2] >= 1) & (pt[:, 2] <= nreg) & (pt[:, 6] != me) & (pt[:, 6] >= 0)
    assert not full_window or (pt[paired, 2] == nreg).sum() >= len(pairs) // 4
    assert paired.sum() >= len(pairs) - solo_ok, [(int(tasks["qlen"][k]), int(tasks["tlen"][k]), pt[k].tolist())
                                                  for k in np.flatnonzero(~paired)[:6]]
    if mixed:
        assert ((pt[paired, 1] >= 130) & (pt[paired, 1] < 140)).all(), sorted(set(pt[:, 1].tolist()))  # the MIXED launch classes
    eng = sedef_amd.Extz2Engine(0, config=settings or {})
    res, cig = eng.align_batch(tasks, pool, want=want)
    n_paired = eng.last_paired()
    eng.close()
    if not mixed:  # (last_paired counts same-geometry pairs)
        assert n_paired >= paired.sum()
    for (q, t), r in zip(pairs, res):
        exp = oracle.extz2(q, t, w=w)
        got = cig[int(r["cigar_off"]):int(r["cigar_off"]) + int(r["n_cigar"])]
        where = (w, len(q), len(t))
        for f in FIELDS:
            assert int(r[f]) == exp[f], (f,) + where + (int(r[f]), exp[f])
        assert np.array_equal(np.asarray(got, np.uint32), np.asarray(exp["cigar"], np.uint32)), \
            where + (cigar_to_str(got), cigar_to_str(exp["cigar"]))
        if not exp["zdropped"]:
            assert {k: int(r[k]) for k in ("matches", "mismatches", "gaps", "gap_bases")} == oracle.counts(exp["cigar"], q, t), where


def _band_lo(r, ql, w):
    return max(0, r - ql + 1, (r - w + 1) >> 1)


def _window_moves(ql, tl, w):
    """How often the window of a task moves: at a block start (every 16 rows) it is re-based to the band start of that row,
    rounded down to 16 slots."""
    base = moves = 0
    for r0 in range(0, ql + tl - 1, 16):
        lo = _band_lo(r0, ql, w) & ~15
        assert lo in (base, base + 16)
        moves += lo != base
        base = lo
    return moves


def _steady_blocks(ql, tl, w, nreg):
    """Block starts r0 at which the kernel runs its steady row flavour: the block predicate of extz2_pair.hip."""
    out, kt, nrow = [], nreg - 1, ql + tl - 1
    for r0 in range(0, nrow, 16):
        base, rl = _band_lo(r0, ql, w) & ~15, r0 + 15
        lo0a, hi0a = (r0 - w + 1) >> 1, (r0 + w) >> 1
        if w >= 2 and r0 + 16 <= nrow and base >= 16 and ((rl - w + 1) >> 1) >= rl - ql + 1 and ((rl + w) >> 1) < tl - 1 and \
                ((r0 + w) >> 1) + 15 < r0 and lo0a + ((w - 1) & ~15) + 16 - base >= 64 * kt and (hi0a | 15) - base >= 64 * kt and \
                hi0a - 1 - base >= 64 * kt - 64:
            out.append(r0)
    return out


def _clip_free(ql, tl, w):  # pair_clip_free of extz2_geom.h
    return min(2 * ql - w - 2, max(tl - 2, 2 * tl - w - 3))


def _shared_rows(qa, ta, qb, tb, w):  # pair_shared_rows of extz2_geom.h
    c = min(_clip_free(qa, ta, w), _clip_free(qb, tb, w))
    return c // 16 * 16 if c >= 16 else 0


def _pair_of_rows(rng, nrow, skew, w, n_every=0):
    """Two sequences with qlen + tlen - 1 == nrow, the query `skew` bases longer than half; n_every > 0: an N every so many
    bases of both, from different phases."""
    ql = min(max(1, (nrow + 1) // 2 + skew), nrow)
    tl = nrow + 1 - ql
    assert abs(ql - tl) <= w  # the band reaches the end: not the TRACK flavour
    q = random_codes(rng, ql)
    t = mutate(rng, q, 0.05, 0.015, 0.015)
    t = t[:tl] if len(t) >= tl else np.concatenate([t, random_codes(rng, tl - len(t))])
    if n_every:
        q, t = q.copy(), t.copy()
        q[3::n_every] = 4
        t[n_every // 2::n_every] = 4
    return q, t


def _twice(rng, pairs):
    """Every task with a partner of its own geometry and other bases (the two halves of the registers differ)."""
    out = []
    for q, t in pairs:
        q2 = q.copy()
        at = rng.random(len(q2)) < 0.04
        q2[at] = (q2[at] + 1) & 3
        out += [(q, t), (q2, t)]
    return out


def _first_steady_rows(w, nreg):
    """The smallest row count of a balanced task (query and target of _pair_of_rows(n, 0)) that has a steady block."""
    for n in range(32, 8 * (w + 64)):
        ql = (n + 1) // 2
        if _steady_blocks(ql, n + 1 - ql, w, nreg):
            return n
    raise AssertionError("no steady block at w = %d" % w)


@pytest.mark.parametrize("w", sorted(NREG_OF_BAND))
def test_row_counts_at_block_and_period_edges(oracle, w):
    """The row counts at the block and period edges (none of these tasks reaches the steady regime), and around the row
    count at which a task first has a steady block: that one +- 1, and one period later +- 1."""
    rng = np.random.default_rng(7100 + w)
    nreg = NREG_OF_BAND[w]
    first = _first_steady_rows(w, nreg)
    rows = EDGE_ROWS + (first - 1, first, first + 1, first + 31, first + 32, first + 33)
    pairs = [_pair_of_rows(rng, n, s, w) for n in rows for s in (0, 2)]
    assert not any(_steady_blocks(len(q), len(t), w, nreg) for q, t in pairs[:2 * len(EDGE_ROWS)])
    assert not _steady_blocks(*map(len, pairs[2 * len(EDGE_ROWS)]), w, nreg) and _steady_blocks(*map(len, pairs[2 * len(EDGE_ROWS) + 2]), w, nreg)
    _run(oracle, _twice(rng, pairs), w, nreg, full_window=False)


@pytest.mark.parametrize("w", sorted(NREG_OF_BAND))
def test_every_row_count_around_the_first_steady_row(oracle, w):
    """160 consecutive row counts from eight below the first one with a steady block: tasks with no steady block, with one,
    and with whole periods of them; every task's window fills all the band's registers."""
    rng = np.random.default_rng(7200 + w)
    nreg = NREG_OF_BAND[w]
    first = _first_steady_rows(w, nreg)
    pairs = [_pair_of_rows(rng, n, int(rng.integers(0, 4)), w) for n in range(first - 8, first + 152)]
    blocks = [len(_steady_blocks(len(q), len(t), w, nreg)) for q, t in pairs]
    assert blocks.count(0) >= 4 and blocks.count(1) >= 4 and max(blocks) >= 5, blocks
    _run(oracle, _twice(rng, pairs), w, nreg)


@pytest.mark.parametrize("w", sorted(NREG_OF_BAND))
def test_windows_that_move_never_once_and_twice(oracle, w):
    """Thirty tasks each whose window moves never, exactly once, exactly twice and three times, of both query / target
    splits (a target long enough for the third window register, 81 bases, moves its window five times: these are tasks of
    one and two registers at every band); ten or more of them never reach the steady regime."""
    rng = np.random.default_rng(7250 + w)
    nreg = NREG_OF_BAND[w]
    by_moves = {0: [], 1: [], 2: [], 3: []}
    for n in range(20, 2 * w + 200):
        for skew in (0, 3):
            q, t = _pair_of_rows(rng, n, skew, w)
            m = _window_moves(len(q), len(t), w)
            if m in by_moves:
                by_moves[m].append((q, t))
    by_moves = {m: v[:15] + v[15:][-15:] for m, v in by_moves.items()}  # the shortest (fewer registers) and the longest
    assert all(len(v) >= 10 for v in by_moves.values()), {m: len(v) for m, v in by_moves.items()}
    assert sum(not _steady_blocks(len(q), len(t), w, nreg) for v in by_moves.values() for q, t in v) >= 10
    _run(oracle, _twice(rng, [p for v in by_moves.values() for p in v]), w, nreg, full_window=False)


def test_two_task_wavefronts_next_to_a_leftover_task(oracle):
    """Three tasks of every geometry: a pair and one task left over (it runs without a partner of its geometry)."""
    rng = np.random.default_rng(7300)
    pairs = []
    for n in (352, 385, 417, 450):
        for _ in range(3):
            pairs.append(_pair_of_rows(rng, n, 1, 128))
    _run(oracle, pairs, 128, 3, solo_ok=len(pairs) // 3)


@pytest.mark.parametrize("w", sorted(NREG_OF_BAND))
def test_n_in_query_and_target_across_window_moves(oracle, w):
    """An N every seven bases of query and target: a row's band is w + 1 >= 13 cells wide, so in the row of every window
    move some N of either sequence is live.  Every task's window moves, most of them in the steady regime too."""
    rng = np.random.default_rng(7400 + w)
    nreg = NREG_OF_BAND[w]
    first = _first_steady_rows(w, nreg)
    pairs = [_pair_of_rows(rng, n, int(rng.integers(0, 3)), w, n_every=7) for n in range(first - 20, first + 140, 3)]
    assert all(_window_moves(len(q), len(t), w) >= 1 for q, t in pairs)
    assert sum(bool(_steady_blocks(len(q), len(t), w, nreg)) for q, t in pairs) >= len(pairs) // 2
    _run(oracle, _twice(rng, pairs), w, nreg)


def test_mixed_pairs_hand_over_at_both_block_ends_of_the_period(oracle, monkeypatch):
    """Tasks of one band and different lengths, none with a partner of its geometry.  The planner pairs neighbours in the
    order of their last clip-free row; the lengths put the shared row of every other pair on the first block end of the
    32-row period (0 mod 32) and of the pairs between them one block later (16 mod 32)."""
    monkeypatch.setenv("SDF_MIXED_MIN", "2")
    rng = np.random.default_rng(7500)
    w = 128
    lengths = [L for a in range(200, 200 + 24 * 12, 24) for L in (a, a + 8)]
    pairs = [_pair_of_rows(rng, 2 * L - 1, 0, w) for L in lengths]
    tasks, _ = _tasks_of(pairs, w)
    import sedef_amd
    pt = _plan(tasks, sedef_amd.extz2.WANT_CIGAR | sedef_amd.extz2.WANT_SCORE)
    shared = [_shared_rows(len(pairs[k][0]), len(pairs[k][1]), len(pairs[p][0]), len(pairs[p][1]), w)
              for k, p in enumerate(pt[:, 6].tolist()) if k < p]
    assert len(shared) == len(pairs) // 2 and all(s >= 16 and s % 16 == 0 for s in shared), shared
    assert sum(s % 32 == 0 for s in shared) >= 4 and sum(s % 32 == 16 for s in shared) >= 4, shared
    _run(oracle, pairs, w, 3, settings=dict(SDF_MIXED_MIN=2), mixed=True)
