#!/usr/bin/env python3
"""Times sdf_search_extend_device on the inputs of profiles/search_roll.py: a repeat-built query of --mb megabases and a
reference made of its 50 kb blocks, shuffled and mutated; k = 12, w = 16, init_len = 700; no filter array, so every interval
whose roll has jaccard >= 0 is extended.  Needs a GPU; prints the interval count, the share of intervals that came back WIDE
and, per phase, the median of --reps timed windows after one warm-up (profiles/search_windows.py's clock):

  roll, device form     sdf_search_roll_device on the same intervals -- the replay in front of every extension is this walk
  extend, device form   sdf_search_extend_device on arrays that lie in HBM, to the end of its stream
  extend, host 1 thread sdf_search_extend_host on one thread, on the intervals of the first windows alone (--host-intervals of
                        them: an extension over tens of kilobases costs the map milliseconds), given per interval like the others

The limit table is a stand-in for relaxed_jaccard_estimate (the library takes the table from its caller):
limit[s] = max(1, s // 6).  Write the output to profiles/search_extend.txt."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))

import search_roll as SR  # noqa: E402
import search_windows as SW  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=float, default=0.3)
    ap.add_argument("--host-intervals", type=int, default=1500)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--init-len", type=int, default=700)
    ap.add_argument("--window-ms", type=float, default=200.0)
    a = ap.parse_args()
    SW.WINDOW_MS = a.window_ms
    import ctypes as C
    import sedef_amd
    from sedef_amd import extz2
    if not torch.cuda.is_available():
        sys.exit("no GPU: NOT MEASURED")
    eng = sedef_amd.Extz2Engine(0)
    rng = np.random.default_rng(1)
    seq_q = SW.sequence(rng, int(a.mb * 1e6))
    seq_r = SR.reference_of(rng, seq_q)
    eng.pool_upload(seq_q + seq_r)
    q_rng, r_rng = eng.minim_ranges([(0, len(seq_q))]), eng.minim_ranges([(len(seq_q), len(seq_r))])
    _, q = eng.pool_minimizers(q_rng)
    _, r = eng.pool_minimizers(r_rng)
    _, r_sorted, _, threshold = eng.pool_minimizer_index(r_rng)
    limit = np.array([max(1, s // 6) for s in range(8192)], np.int32)
    code, first, windows, intervals, used = eng.search_windows_raw(q, r_sorted, int(threshold[0]), len(seq_q), a.init_len, 0, 1, limit)
    assert code == 0
    intervals = intervals[:used]
    code, rolls = eng.search_roll_raw(q, windows, first, intervals, r, len(seq_r), a.init_len, limit)
    assert code == 0
    args = (q, windows, first, intervals, rolls, None, r, len(seq_q), len(seq_r), a.init_len, limit)

    def up(x):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).cuda()
    d = [up(q), up(windows), up(first.astype(np.uint64)), up(intervals), up(r), up(limit), up(rolls)]
    d_roll = torch.zeros(used * 24, dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(used * 40, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    P = extz2.extend_params()

    def roll_call():
        assert eng.lib.sdf_search_roll_device(eng.ctx, d[0].data_ptr(), len(q), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), used,
                                              d[4].data_ptr(), len(r), len(seq_r), a.init_len, d[5].data_ptr(), len(limit),
                                              d_roll.data_ptr(), None) == 0

    def extend_call():
        assert eng.lib.sdf_search_extend_device(eng.ctx, d[0].data_ptr(), len(q), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                                                d[6].data_ptr(), None, used, d[4].data_ptr(), len(r), len(seq_q), len(seq_r), a.init_len,
                                                d[5].data_ptr(), len(limit), C.byref(P), d_out.data_ptr(), None) == 0
    print("%d intervals" % used, file=sys.stderr, flush=True)
    rows = [("roll, device form", SW.median_ms(roll_call, a.reps), used)]
    print("roll timed", file=sys.stderr, flush=True)
    rows.append(("extend, device form", SW.median_ms(extend_call, a.reps), used))
    print("extend timed", file=sys.stderr, flush=True)
    dev = np.frombuffer(d_out.cpu().numpy().tobytes(), extz2.SEARCH_HIT_DTYPE)
    # the host form on the first windows' intervals: first[] cut there, so the windows behind them have none
    cut = int(first[np.searchsorted(first, min(used, a.host_intervals), "right") - 1])
    head = (q, windows, np.minimum(first, cut), intervals, rolls, None, r, len(seq_q), len(seq_r), a.init_len, limit)
    rows.append(("extend, host 1 thread", SW.median_ms(lambda: extz2.search_extend_host(*head), 1), cut))
    code, want = extz2.search_extend_host(*head)
    want = want[:cut]
    dev, rolls_all, used_all, used = dev[:cut], rolls, used, cut
    wide_all = (np.frombuffer(d_out.cpu().numpy().tobytes(), extz2.SEARCH_HIT_DTYPE)["flags"] & extz2.EXTEND_WIDE) != 0
    rolls = rolls[:cut]
    wide = (want["flags"] & extz2.EXTEND_WIDE) != 0
    assert code == 0 and dev[~wide].tobytes() == want[~wide].tobytes() and (dev["flags"][wide] == extz2.EXTEND_WIDE).all()
    ran = (want["flags"] & (extz2.EXTEND_SKIPPED | extz2.EXTEND_NOLIMIT)) == 0
    grew = np.maximum(want["q_winnow_end"].astype(np.int64) - want["q_winnow_start"] - windows["n_members"][np.searchsorted(first, np.arange(used), "right") - 1],
                      want["r_winnow_end"].astype(np.int64) - want["r_winnow_start"] - (rolls["winnow_end"].astype(np.int64) - rolls["winnow_start"]))
    length = want["query_end"].astype(np.int64) - want["query_start"]
    print("query %.2f Mb, reference %.2f Mb, k 12, w 16, init_len %d: %d + %d minimizers, threshold %d"
          % (len(seq_q) / 1e6, len(seq_r) / 1e6, a.init_len, len(q), len(r), int(threshold[0])))
    entered = int(((want["flags"] & extz2.EXTEND_SKIPPED) == 0).sum())
    print("the host form's %d intervals: %d entered the extension, %d of them WIDE (%.2f %%), %d beyond the limit table (after the "
          "growth: WIDE | NOLIMIT); of the %d with a hit: length mean %.0f max %d; records added per hit mean %.1f max %d"
          % (used, entered, int(wide.sum()), 100.0 * wide.sum() / max(1, entered), int((want["flags"] & extz2.EXTEND_NOLIMIT != 0).sum()),
             int(ran.sum()), length[ran].mean() if ran.any() else 0, length[ran].max() if ran.any() else 0,
             grew[ran].mean() if ran.any() else 0, grew[ran].max() if ran.any() else 0))
    print("all %d intervals on the device: WIDE %d (%.2f %%)" % (used_all, int(wide_all.sum()), 100.0 * wide_all.sum() / max(1, used_all)))
    for name, (med, lo, hi), n in rows:
        print("%-22s median %10.2f ms   (min %.2f, max %.2f)   %d intervals, %.2f us each" % (name, med, lo, hi, n, 1e3 * med / max(1, n)))
    per = [med / max(1, n) for _, (med, _, _), n in rows]
    print("the roll's walk is %.0f %% of the extension's time; the host form takes %.1f times the device form per interval"
          % (100.0 * per[0] / per[1], per[2] / per[1]))


if __name__ == "__main__":
    main()
