"""GPU: what a context holds on the device and what it leaves behind (sdf_ctx.h: the table of device buffers).

sdf_debug_live_device_bytes counts, for the process, the bytes the contexts' buffers obtained minus the bytes they gave
back: the device's free memory is everybody's on a shared machine, this figure is exact.  One small call of every kind that
owns buffers, then
  * the counter's rise equals sdf_device_bytes of the context, to the byte: sdf_device_bytes misses no buffer;
  * after sdf_destroy the counter is where it was, to the byte: sdf_destroy misses no buffer.
(The counter is the process's: contexts other tests left alive are idle meanwhile, so the checks read its rise over the
value it had when the test began.)"""
import gc

import numpy as np
import pytest

from oracle.binding import cigar_to_str, mutate, random_codes

pytestmark = pytest.mark.gpu

LETTERS = np.frombuffer(b"ACGTN", np.uint8)


@pytest.fixture(scope="module")
def inputs():
    """The inputs of one round of calls, made once: (lane pairs, stripe pairs, anchor pairs, FASTA record)."""
    rng = np.random.default_rng(20250)
    lane = []
    for _ in range(2000):
        q = random_codes(rng, int(rng.integers(8, 61)))
        lane.append((q, mutate(rng, q)[:60]))
    stripe = []
    for _ in range(4):
        q = random_codes(rng, 600)
        stripe.append((q, (mutate(rng, q, 0.03, 0.0, 0.0))[:600]))
    anchors = []
    for _ in range(2):
        q = random_codes(rng, 200)
        anchors.append((LETTERS[q].tobytes().decode(), LETTERS[mutate(rng, q, 0.02, 0.0, 0.0)].tobytes().decode(), 0, 0))
    rec = LETTERS[random_codes(rng, 100)].tobytes()
    return lane, stripe, anchors, rec[:60] + b"\n" + rec[60:] + b"\n"


def _round(oracle, inputs, check_results):
    """One context, one call of each kind that owns device buffers.  Returns the engine (open)."""
    import sedef_amd
    from sedef_amd.extz2 import TASK_DTYPE, WANT_CIGAR, WANT_SCORE
    lane, stripe, anchor_pairs, fasta = inputs
    # (the lane kernel takes batches of SDF_LANE_MIN tasks and more: 8,192 unless the context says otherwise)
    eng = sedef_amd.Extz2Engine(0, workspace_bytes=256 << 20, config=dict(SDF_LANE_MIN=1024))
    # lane-sized tasks without sdf_reserve: the launch path sizes ln_bins
    res, cig = eng.align_pairs(lane, w=-1, want=WANT_CIGAR | WANT_SCORE)
    assert eng.last_lane_tasks() > 0
    # full-band tasks of 600 x 600 (claim_buf)
    res_s, cig_s = eng.align_pairs(stripe, w=-1, want=WANT_CIGAR | WANT_SCORE)
    # the stats columns of three short alignments (st_items)
    alns = [(LETTERS[q].tobytes(), LETTERS[t].tobytes(), cig[int(r["cigar_off"]):int(r["cigar_off"]) + int(r["n_cigar"])])
            for (q, t), r in zip(lane[:3], res[:3])]
    cols = eng.stats_columns_batch(alns)
    found = eng.anchors_batch(anchor_pairs)
    assert all(len(a) > 0 for a in found)
    chains = eng.chain_batch([np.array(a, np.int32) for a in found])
    assert eng.pool_append_fasta(fasta, 100, 60, 61, reset=True) == 0
    tasks = np.zeros(1, TASK_DTYPE)
    tasks[0] = (0, 50, 50, 50, -1, -1, 0, 0)
    brief, cig_p = eng.align_batch_pairs(tasks)
    if check_results:  # (the calls did their work: a few of each against the oracle)
        for pairs, rr, cc in ((lane[:8], res, cig), (stripe[:1], res_s, cig_s)):
            for (q, t), r in zip(pairs, rr):
                exp = oracle.extz2(q, t, w=-1)
                assert int(r["score"]) == exp["score"]
                assert cigar_to_str(cc[int(r["cigar_off"]):int(r["cigar_off"]) + int(r["n_cigar"])]) == cigar_to_str(exp["cigar"])
        for (a, b, runs), c in zip(alns, cols):
            assert [int(c[f]) for f in cols.dtype.names] == oracle.stats_columns(a, b, runs).tolist()
        for a, (path, bounds) in zip(found, chains):
            exp = oracle.chain_anchors(np.array(a, np.int32))
            assert np.array_equal(path, exp["path"]) and np.array_equal(bounds, exp["bounds"])
        assert int(brief["n_cigar"][0]) > 0
    return eng


def test_nothing_survives_destroy(oracle, inputs):
    from sedef_amd.extz2 import live_device_bytes
    gc.collect()  # (an engine nobody refers to any more goes now, not in the middle of the test)
    base = live_device_bytes()
    eng = _round(oracle, inputs, check_results=True)
    held = eng.device_bytes()
    assert held > 256 << 10
    assert live_device_bytes() - base == held
    eng.close()
    assert live_device_bytes() == base


def test_sixteen_cycles_leave_nothing(oracle, inputs):
    from sedef_amd.extz2 import live_device_bytes
    gc.collect()
    base = live_device_bytes()
    for it in range(16):
        eng = _round(oracle, inputs, check_results=False)
        assert live_device_bytes() - base == eng.device_bytes(), it
        eng.close()
        assert live_device_bytes() == base, it


def test_device_bytes_sees_the_stats_list():
    """The segment list of the stats kernels -- stats_items records of a task and two words -- is part of what the context
    holds."""
    import sedef_amd
    from sedef_amd.extz2 import STATS_TASK_DTYPE
    cfg = sedef_amd.Config()
    eng = sedef_amd.Extz2Engine(0, config=cfg)
    before = eng.device_bytes()
    a = b"ACGTACGTAC"
    cols = eng.stats_columns_batch([(a, a, np.array([len(a) << 4], np.uint32))])
    assert int(cols["matches"][0]) == len(a)
    items = int(cfg.as_dict()["SDF_STATS_ITEMS"])
    assert items >= 1
    assert eng.device_bytes() - before >= items * (STATS_TASK_DTYPE.itemsize + 8)
    eng.close()
