#!/usr/bin/env python3
"""Times the long form of the search extension on the inputs of profiles/search_extend.py at its defaults (a repeat-built query
of --mb megabases against its own shuffled, mutated 50 kb blocks; k = 12, w = 16, init_len = 700; no filter array).  Needs a
GPU; prints, after one warm-up, the median of --reps runs of

  extend, short form      sdf_search_extend_device on arrays that lie in HBM
  extend, long form       sdf_search_extend_long_device behind it (long_grow = 16,384, every candidate, the default batch), with
                          the share of the intervals that are still uncompleted afterwards
  sdf_search_extend       the whole host-array call: uploads, both device forms, the copies back, the host completion of what
                          is left

and the long form's time per candidate against the host form's per interval (profiles/search_extend.txt: 1.8 ms on one
thread).  The limit table is search_extend.py's stand-in with --limit entries (8,192 there: every long growth then ends at the
table, WIDE | NOLIMIT; a longer table lets the walks run to their hits).

  --whole-call   sdf_search_extend alone, --reps times after a warm-up, one line.  This mode uses nothing this commit added, so
                 the same file runs against a checkout of the parent commit (--root: that checkout) -- alternate the two.
  --trace-run    the short and the long form, twice, nothing else: the run to put under
                 `rocprofv3 --kernel-trace --stats -d DIR -o long -- python profiles/search_extend_long.py --trace-run`
  --stages CSV   reads that run's kernel_stats CSV and prints the long form's kernel time by stage (select, keys, sort, slots,
                 walk); no GPU needed.  hipCUB's scan kernels serve two stages: the selection's scan runs once a call over the
                 records, the slots' scan once a batch over the batch's entries, so the calls are split by their count.

Write the output to profiles/search_extend_long.txt."""
import argparse
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if "--root" in sys.argv:  # the checkout whose library is measured (default: this file's)
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))

import search_roll as SR  # noqa: E402
import search_windows as SW  # noqa: E402


def stages(path):
    """The long form's kernels of a rocprofv3 kernel_stats CSV, by stage."""
    import csv
    rows = [(r["Name"], int(r["Calls"]), int(r["TotalDurationNs"])) for r in csv.DictReader(open(path))]
    split = {"select": 0, "keys": 0, "sort": 0, "slots": 0, "walk": 0}
    other = []
    own = {"search_extend_long_flag_kernel": "select", "search_extend_long_list_kernel": "select", "search_extend_long_keys_kernel": "keys",
           "search_extend_long_heads_kernel": "slots", "search_extend_long_slots_kernel": "slots", "search_extend_long_kernel": "walk"}
    calls = max([c for name, c, _ in rows if "search_extend_long_flag_kernel" in name] + [1])
    batches = max([c for name, c, _ in rows if "search_extend_long_keys_kernel" in name] + [1])
    for name, c, ns in rows:
        mine = [st for key, st in own.items() if "sdf::" + key + "(" in name]
        if mine:
            split[mine[0]] += ns
        elif "radix" in name.lower() or "onesweep" in name.lower() or "histogram" in name.lower():
            split["sort"] += ns
        elif "scan" in name.lower() or "lookback" in name.lower():
            # (the selection's scan: `calls` of its launches; the rest are the batches')
            per = ns / max(1, c)
            n_sel = min(c, calls * max(1, round(c / (calls + batches))))
            split["select"] += int(per * n_sel)
            split["slots"] += ns - int(per * n_sel)
        else:
            other.append((name, c, ns))
    total = sum(split.values())
    print("the long form's kernels, %d calls, %d batches in all: %.2f ms a call" % (calls, batches, total / 1e6 / calls))
    for st, ns in split.items():
        print("  %-7s %10.2f ms a call   %5.1f %%" % (st, ns / 1e6 / calls, 100.0 * ns / max(1, total)))
    for name, c, ns in other:
        print("  (not the long form's: %s, %d calls, %.2f ms)" % (name[:70], c, ns / 1e6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=float, default=0.3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--init-len", type=int, default=700)
    ap.add_argument("--limit", type=int, default=8192)
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--whole-call", action="store_true")
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--stages")
    a = ap.parse_args()
    if a.stages:
        return stages(a.stages)
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
    limit = np.array([max(1, s // 6) for s in range(a.limit)], np.int32)
    code, first, windows, intervals, used = eng.search_windows_raw(q, r_sorted, int(threshold[0]), len(seq_q), a.init_len, 0, 1, limit)
    assert code == 0
    intervals = intervals[:used]
    code, rolls = eng.search_roll_raw(q, windows, first, intervals, r, len(seq_r), a.init_len, limit)
    assert code == 0
    args = (q, windows, first, intervals, rolls, None, r, len(seq_q), len(seq_r), a.init_len, limit)

    def timed(fn, reps):
        ms = []
        for it in range(reps + 1):
            t0 = time.perf_counter()
            fn()
            ms.append(1e3 * (time.perf_counter() - t0))
        return float(np.median(ms[1:])), min(ms[1:]), max(ms[1:])
    if a.whole_call:
        med, lo, hi = timed(lambda: eng.search_extend_raw(*args), a.reps)
        code, hits = eng.search_extend_raw(*args)
        assert code == 0
        print("%-30s median %10.2f ms   (min %.2f, max %.2f)   %d runs after a warm-up, %d intervals, %d of them WIDE, in %s"
              % ("sdf_search_extend, whole call", med, lo, hi, a.reps, used, int((hits["flags"] & extz2.EXTEND_WIDE != 0).sum()), ROOT))
        return

    def up(x):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).cuda()
    d = [up(q), up(windows), up(first.astype(np.uint64)), up(intervals), up(rolls), up(r), up(limit)]
    d_out = torch.zeros(used * 40, dtype=torch.uint8, device="cuda")
    d_left = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    head = (d[0].data_ptr(), len(q), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(), None)
    tail = (d[5].data_ptr(), len(r), len(seq_q), len(seq_r), a.init_len, d[6].data_ptr(), len(limit))

    def short():
        eng.search_extend_device(*head, used, *tail, d_out.data_ptr())  # (stream None: synchronised before it returns)

    def both():
        short()
        eng.search_extend_long_device(*head, used, *tail, d_out.data_ptr(), extz2.EXTEND_LONG_MAX_GROW, None, a.batch, d_left.data_ptr())
    if a.trace_run:
        both()
        both()
        return
    t_short = timed(short, a.reps)
    hits = np.frombuffer(d_out.cpu().numpy().tobytes(), extz2.SEARCH_HIT_DTYPE)
    wide = int(((hits["flags"] == extz2.EXTEND_WIDE) & (hits["query_end"] == 0)).sum())
    t_both = timed(both, a.reps)
    hits = np.frombuffer(d_out.cpu().numpy().tobytes(), extz2.SEARCH_HIT_DTYPE)
    still = int(((hits["flags"] == extz2.EXTEND_WIDE) & (hits["query_end"] == 0)).sum())
    left = int(d_left.cpu()[0])
    t_call = timed(lambda: eng.search_extend_raw(*args), a.reps)
    print("query %.2f Mb, reference %.2f Mb, k 12, w 16, init_len %d, limit table %d: %d intervals" % (len(seq_q) / 1e6, len(seq_r) / 1e6, a.init_len, len(limit), used))
    print("after the short form %d uncompleted (%.2f %%); after the long form %d (%.2f %%), *d_left %d; completed with a hit %d, WIDE | NOLIMIT %d"
          % (wide, 100.0 * wide / max(1, used), still, 100.0 * still / max(1, used), left,
             int(((hits["flags"] == extz2.EXTEND_WIDE) & (hits["query_end"] != 0)).sum()),
             int((hits["flags"] == (extz2.EXTEND_WIDE | extz2.EXTEND_NOLIMIT)).sum())))
    for name, (med, lo, hi) in (("extend, short form", t_short), ("extend, short + long form", t_both), ("sdf_search_extend, whole call", t_call)):
        print("%-30s median %10.2f ms   (min %.2f, max %.2f)" % (name, med, lo, hi))
    print("the long form: %.2f ms for %d candidates, %.1f us each (the host form: 1,778 us an interval on one thread)"
          % (t_both[0] - t_short[0], wide, 1e3 * (t_both[0] - t_short[0]) / max(1, wide)))


if __name__ == "__main__":
    main()
