#!/usr/bin/env python3
"""Times the two tree queries of the search on the inputs of profiles/search_roll.py: a repeat-built query of --mb megabases
and a reference made of its 50 kb blocks, shuffled and mutated; k = 12, w = 16, init_len = 700.  The list of found records is
made up, not replayed: --records of them, each the place of a rolled interval of the empty-tree run widened to --record-len
bases on both axes, every window and every interval seeing the whole list -- the most a query can see.  Needs a GPU; prints,
per phase, the median of --reps timed windows after one warm-up (profiles/search_windows.py's clock):

  windows, empty tree      sdf_search_windows_device
  windows, found records   sdf_search_windows_found_device: the index rebuild, the staged records per window, the test of
                           every gathered position against them (n_gathered * records / 64 steps a window)
  index alone              sdf_search_overlap_device on one interval: three launches for the index and one lane
  overlap                  sdf_search_overlap_device on every rolled interval

NO RESULT FILE IS COMMITTED: nobody has run this on a GPU yet.  Write the output to profiles/search_found.txt."""
import argparse
import ctypes as C
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
    ap.add_argument("--records", type=int, default=2000)
    ap.add_argument("--record-len", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--init-len", type=int, default=700)
    ap.add_argument("--window-ms", type=float, default=200.0)
    a = ap.parse_args()
    SW.WINDOW_MS = a.window_ms
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
    assert code == 0 and used > 0
    intervals = intervals[:used]
    code, rolls = eng.search_roll_raw(q, windows, first, intervals, r, len(seq_r), a.init_len, limit)
    assert code == 0
    # the made-up list: the places of evenly spaced rolled intervals, widened
    owner = np.searchsorted(first, np.arange(used), "right") - 1
    pick = np.linspace(0, used - 1, min(a.records, used)).astype(np.int64)
    found = np.zeros(len(pick), extz2.SEARCH_FOUND_DTYPE)
    found["q_start"] = np.maximum(0, q["loc"][owner[pick]].astype(np.int64) - a.record_len // 2)
    found["q_end"] = found["q_start"].astype(np.int64) + a.record_len
    found["r_start"] = np.maximum(0, rolls["ref_start"][pick].astype(np.int64) - a.record_len // 2)
    found["r_end"] = found["r_start"].astype(np.int64) + a.record_len
    entries = extz2.found_entries(found)
    visible, visible_iv = np.full(len(q), len(found), np.uint32), np.full(used, len(found), np.uint32)

    def up(x):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).cuda()
    d_q, d_r, d_limit, d_found, d_vis, d_viv, d_rolls = up(q), up(r_sorted), up(limit), up(found), up(visible), up(visible_iv), up(rolls)
    d_first = torch.zeros(len(q) + 1, dtype=torch.int64, device="cuda")
    d_win = torch.zeros(len(q) * 20, dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(used * 8, dtype=torch.uint8, device="cuda")
    d_first0 = up(first.astype(np.uint64))
    d_verdict = torch.zeros(used, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    n_used = C.c_size_t(0)
    head = (eng.ctx, d_q.data_ptr(), len(q), len(seq_q), d_r.data_ptr(), len(r_sorted), int(threshold[0]), a.init_len, 0, 1,
            d_limit.data_ptr(), len(limit))
    tail = (d_first.data_ptr(), d_win.data_ptr(), d_out.data_ptr(), used, C.byref(n_used), None)

    def plain_call():
        assert eng.lib.sdf_search_windows_device(*head, *tail) == 0

    def found_call():
        assert eng.lib.sdf_search_windows_found_device(*head, d_found.data_ptr(), len(found), entries, None, d_vis.data_ptr(), *tail) == 0

    def overlap_call(n):
        assert eng.lib.sdf_search_overlap_device(eng.ctx, d_q.data_ptr(), len(q), d_first0.data_ptr(), d_rolls.data_ptr(), n,
                                                 d_found.data_ptr(), len(found), entries, None, d_viv.data_ptr(), a.init_len, a.init_len,
                                                 d_verdict.data_ptr(), None, None) == 0
    rows = [("windows, empty tree", SW.median_ms(plain_call, a.reps), len(q)),
            ("windows, found records", SW.median_ms(found_call, a.reps), len(q))]
    lost = int(windows["n_candidates"].astype(np.int64).sum()) - int(
        np.frombuffer(d_win.cpu().numpy().tobytes(), extz2.SEARCH_WINDOW_DTYPE)["n_candidates"].astype(np.int64).sum())
    wide = int((np.frombuffer(d_win.cpu().numpy().tobytes(), extz2.SEARCH_WINDOW_DTYPE)["flags"] & extz2.SEARCH_FOUND_WIDE != 0).sum())
    rows.append(("index alone", SW.median_ms(lambda: overlap_call(1), a.reps), len(found)))
    rows.append(("overlap", SW.median_ms(lambda: overlap_call(used), a.reps), used))
    ones = int(d_verdict.cpu().numpy().sum())
    print("query %.2f Mb, reference %.2f Mb, k 12, w 16, init_len %d: %d windows, %d rolled intervals; %d found records of %d bases, "
          "%d bin entries" % (len(seq_q) / 1e6, len(seq_r) / 1e6, a.init_len, len(q), used, len(found), a.record_len, entries))
    print("the records take %d candidates from the windows, %d windows are FOUND_WIDE, %d intervals overlap" % (lost, wide, ones))
    for name, (med, lo, hi), n in rows:
        print("%-24s median %10.3f ms   (min %.3f, max %.3f)   %d items, %.3f us each" % (name, med, lo, hi, n, 1e3 * med / max(1, n)))


if __name__ == "__main__":
    main()
