#!/usr/bin/env python3
"""Times sdf_search_filter_device on the pair of profiles/search_roll.py: every rolled interval whose jaccard is at least 0,
against the range where its walk ended (allow_extend on); the reference's default parameters.  Needs a GPU; prints, per phase,
the median of --reps timed windows after one warm-up (profiles/search_windows.py's clock):

  tasks, device         sdf_search_filter_tasks_device: one lane per interval
  device form           sdf_search_filter_device on tasks that lie in HBM, to the end of its stream: the wavefront class's
                        launch and the long class's, whose workgroups all leave at once here
  wavefront class       that first launch alone (sdf_search_filter_phase_device, not in the header, for this script): the
                        difference is what the long class's launch costs over tasks that are not its own
  histogram pass        the same launch with workgroups that leave before the min-sum -- the min-sum's share is the difference
  combined form         sdf_search_filter: the tasks' upload, the launch, the read-back
  host, 1 thread        sdf_search_filter_host on the same tasks
  64 homopolymer tasks  the device form and the host form on 64 pairs of 700 characters cut from one run of 'a', and the
                        device form on 64 pairs of 700 random characters for comparison; then as many of either kind as the
                        pair has live tasks, through the wavefront class's launch

Write the output to profiles/search_filter.txt."""
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
    seq_r = SR.reference_of(rng, seq_q)
    pool = seq_q + seq_r + b"a" * 4096
    eng.pool_upload(pool)
    eng.pool_sync()
    limit = np.array([max(1, s // 6) for s in range(4096)], np.int32)
    first, windows, intervals, rolls = eng.search_roll((0, len(seq_q)), (len(seq_q), len(seq_r)), init_len=a.init_len, limit=limit)
    _, q = eng.pool_minimizers(eng.minim_ranges([(0, len(seq_q))]))
    n = len(intervals)
    targs = (len(seq_q), len(seq_r), a.init_len, 0, 0, len(seq_q), 0, 1)
    code, tasks = extz2.search_filter_tasks_host(q, windows, first, intervals, rolls, *targs)
    assert code == 0
    P = extz2.filter_params()

    def up(x):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).cuda()
    d = [up(q), up(windows), up(first.astype(np.uint64)), up(intervals), up(rolls)]
    d_tasks = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(n * 20, dtype=torch.uint8, device="cuda")
    homo = np.zeros(64, extz2.FILTER_TASK_DTYPE)
    homo["q_off"], homo["r_off"] = len(pool) - 4096 + np.arange(64), len(pool) - 2048 + np.arange(64)
    homo["q_len"] = homo["r_len"] = 700
    d_homo, d_homo_out = up(homo), torch.zeros(64 * 20, dtype=torch.uint8, device="cuda")
    rand = homo.copy()
    rand["q_off"], rand["r_off"] = 1000 * np.arange(64), len(seq_q) + 1000 * np.arange(64)
    d_rand = up(rand)
    # ... and as many of either kind as the pair has live tasks
    many = int(((tasks["flags"] & extz2.FILTER_SKIP) == 0).sum())
    homo_n, rand_n = np.resize(homo, many), np.zeros(many, extz2.FILTER_TASK_DTYPE)
    rand_n["q_off"], rand_n["r_off"] = rng.integers(0, len(seq_q) - 700, many), len(seq_q) + rng.integers(0, len(seq_r) - 700, many)
    rand_n["q_len"] = rand_n["r_len"] = 700
    d_homo_n, d_rand_n = up(homo_n), up(rand_n)
    torch.cuda.synchronize()

    def phase(which):
        assert eng.lib.sdf_search_filter_phase_device(eng.ctx, P, d_tasks.data_ptr(), n, 0, which, d_out.data_ptr(), None) == 0

    def build():
        eng.search_filter_tasks_device(d[0].data_ptr(), len(q), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(), n, *targs,
                                       d_tasks.data_ptr())
    rows = [("tasks, device", SW.median_ms(build, a.reps))]
    assert d_tasks.cpu().numpy().tobytes() == tasks.tobytes()
    rows.append(("device form", SW.median_ms(lambda: eng.search_filter_device(d_tasks.data_ptr(), n, False, d_out.data_ptr(), P), a.reps)))
    dev = np.frombuffer(d_out.cpu().numpy().tobytes(), extz2.FILTER_REC_DTYPE)
    rows.append(("wavefront class", SW.median_ms(lambda: phase(1), a.reps)))
    rows.append(("histogram pass", SW.median_ms(lambda: phase(0), a.reps)))
    rows.append(("combined form", SW.median_ms(lambda: eng.search_filter_raw(tasks, P), a.reps)))
    rows.append(("host, 1 thread", SW.median_ms(lambda: extz2.search_filter_host(pool, tasks, P), max(1, a.reps // 2))))
    code, want = extz2.search_filter_host(pool, tasks, P)
    assert code == 0 and dev.tobytes() == want.tobytes()
    rows.append(("64 homopolymer, device", SW.median_ms(lambda: eng.search_filter_device(d_homo.data_ptr(), 64, False, d_homo_out.data_ptr(), P),
                                                       a.reps)))
    rows.append(("64 random, device", SW.median_ms(lambda: eng.search_filter_device(d_rand.data_ptr(), 64, False, d_homo_out.data_ptr(), P), a.reps)))
    eng.search_filter_device(d_homo.data_ptr(), 64, False, d_homo_out.data_ptr(), P)
    for name, d_n in (("%d homopolymer, wavefront class" % many, d_homo_n), ("%d random, wavefront class" % many, d_rand_n)):
        rows.append((name, SW.median_ms(lambda: eng.lib.sdf_search_filter_phase_device(eng.ctx, P, d_n.data_ptr(), many, 0, 1, d_out.data_ptr(),
                                                                                       None), a.reps)))
    rows.append(("64 homopolymer, host", SW.median_ms(lambda: extz2.search_filter_host(pool, homo, P), a.reps)))
    assert np.frombuffer(d_homo_out.cpu().numpy().tobytes(), extz2.FILTER_REC_DTYPE).tobytes() == extz2.search_filter_host(pool, homo, P)[1].tobytes()
    live = (tasks["flags"] & extz2.FILTER_SKIP) == 0
    print("query %.2f Mb, reference %.2f Mb, k 12, w 16, init_len %d: %d intervals, %d filtered (jaccard >= 0), %d skipped"
          % (len(seq_q) / 1e6, len(seq_r) / 1e6, a.init_len, n, int(live.sum()), int((~live).sum())))
    print("verdicts: pass %d, upper %d, q-gram %d; dist mean %.1f, minqg %d" % (
        int((want["flags"][live] == 0).sum()), int((want["flags"] & extz2.FILTER_UPPER_FAIL != 0).sum()),
        int((want["flags"] & extz2.FILTER_QGRAM_FAIL != 0).sum()), want["dist"][live].mean(), int(want["minqg"][live].max())))
    for name, (med, lo, hi) in rows:
        print("%-40s median %10.3f ms   (min %.3f, max %.3f)" % (name, med, lo, hi))
    ms = {name: med for name, (med, lo, hi) in rows}
    print("histogram pass %.0f %% of the wavefront class's launch, min-sum and verdict %.0f %%; the long class's launch over these tasks: "
          "%.3f ms" % (100 * ms["histogram pass"] / ms["wavefront class"], 100 - 100 * ms["histogram pass"] / ms["wavefront class"],
                       ms["device form"] - ms["wavefront class"]))


if __name__ == "__main__":
    main()
