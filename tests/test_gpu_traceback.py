"""The traceback walk, the CIGAR scan and the compaction (sedef_amd/csrc/traceback.hip) at their group-size edges.

Every CIGAR the library returns passes through that file; the DP tests compare CIGARs of randomly mutated sequences, whose
gap runs are one base long.  Here the inputs are tests/tbgen.py's designed ones -- diagonal, E and F runs of G - 1, G, G + 1,
2G, 2G + 1 cells for both group sizes of the walk (G = 16 and 64), runs that end at the matrix edge inside a group, bands
the path hugs or leaves, CIGARs of more than 64 words forward and reversed, walks that start at the best cell -- on every
direction-flag layout, each forced with the settings of tests/test_gpu_fuzz_slice.py.  Every case compares every result
field its route serves, every CIGAR word and the four column counters with the CPU checker (the reference's own
ksw_extz2_sse where oracle/_ref is present, else the scalar oracle), bit for bit, and asserts through
Extz2Engine.last_traceback_classes() that the intended traceback_kernel<layout, G> was the one launched.

Which group size runs is launch_chunk's decision (sedef_amd/csrc/sdf_launch.hip):

    const bool tb_solo = cnt <= (nchunks == 1 ? (size_t)8192 : (size_t)1024);

so a call of at most 8,192 tasks in one chunk is walked in groups of 64, and the same cases copied into one call of more
than 8,192 tasks in groups of 16.  Reached that way: layouts 0, 1, 2, 3, 4 and 6 with both group sizes (a call in which
every task is "heavy", or none is, has no heavy chunk: the stripe, banded-stripe and strip tasks stay in one chunk of more
than 8,192).  NOT reachable through the ABI:

  * layout 5 with G = 64: the lane path has a launch site of its own, launch_lane, which passes `false` for `solo`
    (`launch_traceback<5>(ctx, false, nl, ...)`, twice) whatever the number of lane tasks;
  * the MIXED flavour of the pair kernel (layout 2) with G = 16 on designed cases: the planner forms mixed pairs from tasks
    without a partner of their own geometry when they are a sixteenth of the chunk (sdf_plan.hip: `keys.size() * 16 < cnt`),
    which copies of a few hundred cases never are.  Layout 2 itself runs with both group sizes (the exact pairs and the
    TRACK flavour), and tb_addr does not know the flavours apart: it reads the task's nreg.

The scan tests cover the record counts around the 1,024 records of a scan block and a call of more than 2^20 tasks (the
second pass of cigar_scan_parts_kernel and its carry)."""
import numpy as np
import pytest
import torch  # (at collection, like the modules that import bench: before the library brings a HIP runtime of its own along)

import tbgen

pytestmark = pytest.mark.gpu

ALL_FIELDS = ("max", "zdropped", "max_q", "max_t", "mqe", "mqe_t", "mte", "mte_q", "score")  # want = 7: the general kernel
FAST_FIELDS = ("score", "mte", "mte_q", "zdropped")  # want = CIGAR | score: the register-resident kernels
COUNTS = ("matches", "mismatches", "gaps", "gap_bases")


@pytest.fixture(scope="module")
def cpu(oracle):
    """The checker: the reference kernel where it was built, else the scalar oracle."""
    from oracle.binding import Reference
    try:
        return Reference()
    except Exception:  # noqa: BLE001  (oracle/_ref is not there)
        return oracle


_EXPECTED = {}


def _expected(cpu, oracle, key, cases):
    """Per case: the checker's record, its CIGAR words and the counters of that CIGAR; computed once per case list."""
    if key not in _EXPECTED:
        out = []
        for c in cases:
            e = cpu.extz2(c.q, c.t, w=c.w, zdrop=c.zdrop, flag=c.flag)
            words = e["cigar"]
            fwd = words[::-1] if c.flag & tbgen.REV_CIGAR else words
            e["counts"] = oracle.counts(fwd, c.q, c.t)
            out.append(e)
        _EXPECTED[key] = out
    return _EXPECTED[key]


def _check_records(res, cig, exp, copies, fields, what):
    """Every record of `copies` copies of the cases against `exp`; the CIGAR pool word for word."""
    def col(f):
        return np.tile(np.array([e[f] for e in exp], np.int64), copies)
    zd = col("zdropped") != 0
    for f in fields:
        bad = np.flatnonzero(res[f].astype(np.int64) != col(f))
        assert len(bad) == 0, (what, f, len(bad), int(bad[0]) % len(exp), int(res[f][bad[0]]), int(col(f)[bad[0]]))
    for f in ("max", "max_t", "max_q"):  # the best cell, where the walk started from it
        bad = np.flatnonzero((res[f].astype(np.int64) != col(f)) & zd)
        assert len(bad) == 0, (what, f, len(bad), int(bad[0]) % len(exp))
    ncig = np.tile(np.array([len(e["cigar"]) for e in exp], np.int64), copies)
    bad = np.flatnonzero(res["n_cigar"].astype(np.int64) != ncig)
    assert len(bad) == 0, (what, "n_cigar", len(bad), int(bad[0]) % len(exp), int(res["n_cigar"][bad[0]]), int(ncig[bad[0]]))
    off = np.concatenate([[0], np.cumsum(ncig)])
    assert np.array_equal(res["cigar_off"].astype(np.int64), off[:-1]), (what, "cigar_off")
    words = np.tile(np.concatenate([e["cigar"] for e in exp]).astype(np.uint32), copies)
    assert len(cig) == off[-1] == len(words), (what, "cigar_used", len(cig), int(off[-1]))
    bad = np.flatnonzero(cig != words)
    if len(bad):
        k = int(np.searchsorted(off, bad[0], side="right") - 1)
        raise AssertionError((what, "CIGAR word", len(bad), k % len(exp), int(bad[0] - off[k]), int(cig[bad[0]]), int(words[bad[0]])))
    for f in COUNTS:
        want = np.tile(np.array([e["counts"][f] for e in exp], np.int64), copies)
        bad = np.flatnonzero(res[f].astype(np.int64) != want)
        assert len(bad) == 0, (what, f, len(bad), int(bad[0]) % len(exp), int(res[f][bad[0]]), int(want[bad[0]]))


def _assert_launched(eng, layout, G, what):
    cls = eng.last_traceback_classes()
    idx = 2 * layout + (G == 16)
    print("%s: last_traceback_classes %s" % (what, cls))
    assert cls[idx] >= 1, (what, "traceback_kernel<%d, %d> was not launched" % (layout, G), cls)
    # ... and no task went to another layout's kernel.  (The other group size of the SAME layout may run next to it: the few
    # long tasks of a call of thousands leave for a heavy chunk of their own, small enough to be walked in groups of 64.
    # A re-run of tasks a stripe kernel gave up walks them on other layouts.)
    if eng.last_reran() == 0:
        assert {k // 2 for k, v in enumerate(cls) if v} == {layout}, (what, cls)


@pytest.mark.parametrize("route, G", tbgen.CALLS, ids=["%s-G%d" % c for c in tbgen.CALLS])
def test_designed_runs_on_every_layout_and_group_size(cpu, oracle, route, G):
    import sedef_amd
    R = tbgen.ROUTES[route]
    cases, copies, tasks, pool = tbgen.call_tasks(route, G)
    exp = _expected(cpu, oracle, (route, G), cases)
    eng = sedef_amd.Extz2Engine(0, config=R["settings"])
    try:
        res, cig = eng.align_batch(tasks, pool, want=R["want"])
        what = "%s, G = %d, %d cases x %d" % (route, G, len(cases), copies)
        _assert_launched(eng, R["layout"], G, what)
        _check_records(res, cig, exp, copies, ALL_FIELDS if R["want"] == 7 else FAST_FIELDS, what)
        if route == "lane":
            assert eng.last_lane_tasks() == len(tasks)
    finally:
        eng.close()


def _family5_call():
    rng = np.random.default_rng(555)
    cases = tbgen.family5(rng) + [tbgen.family5_even(rng, 64, f) for f in (0, tbgen.REV_CIGAR)] + tbgen.family5(rng, w=16)
    tasks, pool = tbgen.tasks_of(cases, 2)
    return cases, 2, tasks, pool


@pytest.mark.parametrize("form", ["brief", "device"])
def test_many_runs_forward_and_reversed_brief_and_device_forms(cpu, oracle, form):
    """CIGARs of 63, 64, 65, 129 and 131 words, forward and KSW_EZ_REV_CIGAR (the compaction's `c += 64` loop), through
    sdf_extz2_batch_brief and sdf_extz2_batch_device."""
    import sedef_amd
    from sedef_amd import RESULT_DTYPE
    cases, copies, tasks, pool = _family5_call()
    exp = _expected(cpu, oracle, "family5", cases)
    words = np.tile(np.concatenate([e["cigar"] for e in exp]).astype(np.uint32), copies)
    ncig = np.tile(np.array([len(e["cigar"]) for e in exp], np.int64), copies)
    off = np.concatenate([[0], np.cumsum(ncig)])
    assert {63, 64, 65, 129, 131} <= set(ncig.tolist())
    eng = sedef_amd.Extz2Engine(0)
    try:
        if form == "brief":
            res, cig = eng.align_batch_brief(tasks, pool)
            assert np.array_equal(res["n_cigar"], ncig) and np.array_equal(res["cigar_off"], off[:-1])
            assert np.array_equal(cig, words)
            assert np.array_equal(res["matches"], np.tile([e["counts"]["matches"] for e in exp], copies))
        else:
            dev = torch.device("cuda", 0)
            dt, packed, at = tasks.copy(), [], 0
            for k, c in enumerate(cases):  # sequences packed (sdf_pack_codes) in HBM, word offsets
                for side, s in (("q_off", c.q), ("t_off", c.t)):
                    w = sedef_amd.pack_codes(s)
                    dt[side][k::len(cases)] = at
                    packed.append(w)
                    at += len(w)
            d_pool = torch.from_numpy(np.concatenate(packed).view(np.int32)).to(dev)
            cap = int(off[-1]) + 7
            d_out = torch.zeros(len(dt) * 16, dtype=torch.int32, device=dev)
            d_cig = torch.full((cap,), -1, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            used = eng.align_batch_device(dt, d_pool.data_ptr(), d_out.data_ptr(), d_cig.data_ptr(), cap, want=3)
            torch.cuda.synchronize()
            assert used == off[-1]
            got = d_cig.cpu().numpy().view(np.uint32)
            assert (got[used:] == 0xffffffff).all()  # nothing written behind the CIGARs
            _check_records(d_out.cpu().numpy().view(RESULT_DTYPE), got[:used], exp, copies, FAST_FIELDS, "device form")
        assert sum(eng.last_traceback_classes()) >= 1
    finally:
        eng.close()


def _fnv_tasks(res, cig):
    """FNV-1a over each task's CIGAR words (what the checkers' batch calls return), all tasks at once."""
    n = len(res)
    h = np.full(n, 1469598103934665603, np.uint64)
    off, cnt = res["cigar_off"].astype(np.int64), res["n_cigar"].astype(np.int64)
    words = cig.astype(np.uint64)
    with np.errstate(over="ignore"):
        for j in range(int(cnt.max()) if n else 0):
            live = np.flatnonzero(cnt > j)
            h[live] = (h[live] ^ words[off[live] + j]) * np.uint64(1099511628211)
    return h


def _check_scan(res, cig, score_only):
    """cigar_off is the exclusive cumulative sum of n_cigar in record order, cigar_used the total."""
    ncig = res["n_cigar"].astype(np.int64)
    assert (ncig >= 0).all() and (ncig[score_only] == 0).all() and (ncig[~score_only] > 0).all()
    off = np.cumsum(ncig) - ncig
    bad = np.flatnonzero(res["cigar_off"].astype(np.int64) != off)
    assert len(bad) == 0, ("cigar_off", len(bad), int(bad[0]), int(res["cigar_off"][bad[0]]), int(off[bad[0]]))
    assert len(cig) == int(ncig.sum())


def _small_batch(n, seed, hi):
    import bench
    import sedef_amd
    rng = np.random.default_rng(seed)
    ql = rng.integers(1, hi + 1, n)
    tl = rng.integers(1, hi + 1, n)
    pool, q_off, qlen, t_off, tlen = bench.synth_ragged(rng, ql, tl, sub=0.1, dele=0.05, ins=0.05)
    tasks = np.zeros(n, sedef_amd.TASK_DTYPE)
    tasks["q_off"], tasks["t_off"], tasks["qlen"], tasks["tlen"] = q_off, t_off, qlen, tlen
    tasks["w"], tasks["zdrop"] = -1, -1
    return tasks, pool


def _check_against_batch(cpu, tasks, pool, res, cig, score_only):
    """Every task's score, and the FNV-1a hash of its CIGAR, against the checker's batch call."""
    score, h = cpu.batch(pool, tasks["q_off"], tasks["qlen"], tasks["t_off"], tasks["tlen"], w=-1)
    bad = np.flatnonzero(res["score"] != score)
    assert len(bad) == 0, ("score", len(bad), int(bad[0]))
    got = _fnv_tasks(res, cig)
    bad = np.flatnonzero((got != h) & ~score_only)
    assert len(bad) == 0, ("CIGAR hash", len(bad), int(bad[0]))


@pytest.mark.parametrize("n", [1023, 1024, 1025, 2049])
def test_scan_record_counts_around_a_block(cpu, n):
    """Calls of 1,023, 1,024, 1,025 and 2,049 tasks, every third of them score-only (no CIGAR: n_cigar 0) between the
    others: the blocks of cigar_scan_blocks_kernel full, one short, one over, and a third block of one record."""
    import sedef_amd
    tasks, pool = _small_batch(n, 1000 + n, 40)
    score_only = np.arange(n) % 3 == 1
    tasks["flag"][score_only] = tbgen.SCORE_ONLY
    eng = sedef_amd.Extz2Engine(0)
    try:
        res, cig = eng.align_batch(tasks, pool, want=3)
    finally:
        eng.close()
    _check_scan(res, cig, score_only)
    _check_against_batch(cpu, tasks, pool, res, cig, score_only)


def test_scan_beyond_two_to_the_twenty_records(cpu):
    """One call of 1,100,000 tasks of 1..6 bases: 1,075 scan blocks, so cigar_scan_parts_kernel's loop runs a second pass
    and its carry is used -- the suite's largest call so far (1,000,000 tasks, 977 blocks) never got there."""
    import sedef_amd
    n = 1100000
    tasks, pool = _small_batch(n, 2 ** 20, 6)
    eng = sedef_amd.Extz2Engine(0)
    try:
        res, cig = eng.align_batch(tasks, pool, want=3)
        print("2^20 call: last_traceback_classes %s, lane tasks %d" % (eng.last_traceback_classes(), eng.last_lane_tasks()))
    finally:
        eng.close()
    none = np.zeros(n, bool)
    _check_scan(res, cig, none)
    _check_against_batch(cpu, tasks, pool, res, cig, none)
