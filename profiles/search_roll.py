#!/usr/bin/env python3
"""Times sdf_search_roll_device on a pair of chromosome-like sequences: a repeat-built query of --mb megabases and a reference
made of its 50 kb blocks, shuffled and mutated; k = 12, w = 16, init_len = 700.  Needs a GPU; prints the interval count and,
per phase, the median of --reps timed windows after one warm-up (profiles/search_windows.py's clock: a timed window repeats
its call until it is at least --window-ms long and reports the time per call):

  device form           sdf_search_roll_device on arrays that lie in HBM, to the end of its stream
  set-up alone          the same launch with wavefronts that leave after gather, sort and slots (sdf_search_roll_setup_device:
                        not in the header, for this script) -- the walk's share is the difference
  combined form         sdf_search_roll: uploads, the launch, the read-back, WIDE intervals completed on the host
  host, 1 thread        sdf_search_roll_host on the same arrays, one thread

The limit table is a stand-in for relaxed_jaccard_estimate (the library takes the table from its caller):
limit[s] = max(1, s // 6).  Write the output to profiles/search_roll.txt."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))

import search_windows as SW  # noqa: E402


def reference_of(rng, seq, block=50000, rate=0.03):
    """The query's blocks in another order, with substitutions at `rate`."""
    a = np.frombuffer(seq, np.uint8).copy()
    blocks = [a[at:at + block] for at in range(0, len(a), block)]
    a = np.concatenate([blocks[j] for j in rng.permutation(len(blocks))])
    hit = np.flatnonzero(rng.random(len(a)) < rate)
    a[hit] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, len(hit))] | (a[hit] & 0x20)
    return a.tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=float, default=3.0)
    ap.add_argument("--reps", type=int, default=5)
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
    seq_r = reference_of(rng, seq_q)
    eng.pool_upload(seq_q + seq_r)
    q_rng, r_rng = eng.minim_ranges([(0, len(seq_q))]), eng.minim_ranges([(len(seq_q), len(seq_r))])
    _, q = eng.pool_minimizers(q_rng)
    _, r = eng.pool_minimizers(r_rng)
    _, r_sorted, _, threshold = eng.pool_minimizer_index(r_rng)
    limit = np.array([max(1, s // 6) for s in range(4096)], np.int32)
    code, first, windows, intervals, used = eng.search_windows_raw(q, r_sorted, int(threshold[0]), len(seq_q), a.init_len, 0, 1, limit)
    assert code == 0
    intervals = intervals[:used]
    args = (q, windows, first, intervals, r, len(seq_r), a.init_len, limit)

    def up(x):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).cuda()
    d = [up(q), up(windows), up(first.astype(np.uint64)), up(intervals), up(r), up(limit)]
    d_out = torch.zeros(used * 24, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def device_call(fn):
        rc = fn(eng.ctx, d[0].data_ptr(), len(q), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), used, d[4].data_ptr(), len(r),
                len(seq_r), a.init_len, d[5].data_ptr(), len(limit), d_out.data_ptr(), None)
        assert rc == 0
    rows = [("set-up alone", SW.median_ms(lambda: device_call(eng.lib.sdf_search_roll_setup_device), a.reps)),
            ("device form", SW.median_ms(lambda: device_call(eng.lib.sdf_search_roll_device), a.reps))]
    dev = np.frombuffer(d_out.cpu().numpy().tobytes(), extz2.SEARCH_ROLL_DTYPE)
    rows.append(("combined form", SW.median_ms(lambda: eng.search_roll_raw(*args), a.reps)))
    rows.append(("host, 1 thread", SW.median_ms(lambda: extz2.search_roll_host(*args), max(1, a.reps // 2))))
    code, want = extz2.search_roll_host(*args)
    wide = (want["flags"] & extz2.ROLL_WIDE) != 0
    assert code == 0 and dev[~wide].tobytes() == want[~wide].tobytes()
    span = want["winnow_end"].astype(np.int64) - want["winnow_start"]
    length = intervals["end"].astype(np.int64) - intervals["start"]
    print("query %.2f Mb, reference %.2f Mb, k 12, w 16, init_len %d: %d + %d minimizers, threshold %d"
          % (len(seq_q) / 1e6, len(seq_r) / 1e6, a.init_len, len(q), len(r), int(threshold[0])))
    print("intervals: %d, WIDE %d; length mean %.1f max %d; best window's records mean %.1f max %d; moved off the start %d; "
          "jaccard >= 0: %d" % (used, int(wide.sum()), length.mean(), length.max(), span.mean(), span.max(),
                                int((want["ref_start"] != intervals["start"]).sum()), int((want["jaccard"] >= 0).sum())))
    for name, (med, lo, hi) in rows:
        print("%-18s median %10.2f ms   (min %.2f, max %.2f)" % (name, med, lo, hi))
    setup, whole = rows[0][1][0], rows[1][1][0]
    print("the walk: %.2f ms, %.0f %% of the device form" % (whole - setup, 100.0 * (whole - setup) / whole))


if __name__ == "__main__":
    main()
