#!/usr/bin/env python3
"""Times sdf_search_windows on a chromosome-like sequence against itself (same_genome): repeat-built, --mb megabases, k = 12,
w = 16, init_len = 700.  Needs a GPU; prints, per phase, the median of --reps timed windows after one warm-up.  A timed
window repeats its call until it is at least --window-ms long (0.2 s) and reports the time per call:

  minimizers / index    sdf_pool_minimizers, sdf_pool_minimizer_index on the resident sequence
  host form             sdf_search_windows: uploads, every launch, the read-back, WIDE windows completed on the host
  device form           sdf_search_windows_device on arrays that lie in HBM, to the end of its stream (a host clock around a
                        call that ends in a synchronise)
  host, 1 thread        sdf_search_windows_host on one thread
  host, 16 threads      the same on 16 threads, each a contiguous share of the windows (its slice of q runs on to the last
                        member of its last window; the windows behind the share are computed and thrown away)

and the share of WIDE windows.  The time per KERNEL comes from a run of its own under the profiler, which slows the host:

  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python profiles/search_windows.py --kernels 20

(--kernels N: N device-form calls and nothing else; DIR/.../run_kernel_stats.csv lists the search_* kernels, the library sort's
and the scan).  The limit table is a stand-in for relaxed_jaccard_estimate (the library takes the table
from its caller): limit[s] = max(1, s // 6).  Write the output to profiles/search_windows.txt."""
import argparse
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sequence(rng, total):
    """Random bases with mutated copies of repeat units of 300 to 6,000 bases, a unit per 30 kb, about five copies of each:
    about half the sequence."""
    units = [rng.integers(0, 4, int(n)) for n in rng.integers(300, 6000, max(20, total // 30000))]
    parts, have = [], 0
    while have < total:
        u = units[int(rng.integers(0, len(units)))].copy()
        hit = rng.random(len(u)) < 0.05
        u[hit] = (u[hit] + rng.integers(1, 4, int(hit.sum()))) % 4
        gap = rng.integers(0, 4, int(rng.integers(200, 6000)))
        parts += [gap, u]
        have += len(gap) + len(u)
    s = np.frombuffer(b"ACGT", np.uint8)[np.concatenate(parts)[:total]].copy()
    for at in rng.integers(0, total - 3000, total // 20000):  # soft-masked stretches
        s[at:at + int(rng.integers(100, 3000))] |= 0x20
    return s.tobytes()


WINDOW_MS = 200.0


def median_ms(f, reps):
    """ms per call of f: the median, minimum and maximum over `reps` timed windows of at least WINDOW_MS each."""
    f()
    t0 = time.perf_counter()
    f()
    inner = max(1, int(np.ceil(WINDOW_MS / max(1e-3, (time.perf_counter() - t0) * 1e3))))
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(inner):
            f()
        times.append((time.perf_counter() - t0) * 1e3 / inner)
    return float(np.median(times)), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=float, default=3.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--init-len", type=int, default=700)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--kernels", type=int, default=0, help="only this many device-form calls: for a run under the profiler")
    a = ap.parse_args()
    global WINDOW_MS
    WINDOW_MS = a.window_ms
    import sedef_amd
    from sedef_amd import extz2
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing is measured without one")
    eng = sedef_amd.Extz2Engine(0)
    seq = sequence(np.random.default_rng(1), int(a.mb * 1e6))
    eng.pool_upload(seq)
    rng_q = eng.minim_ranges([(0, len(seq))])
    rows = []
    if not a.kernels:
        rows.append(("minimizers", median_ms(lambda: eng.pool_minimizers(rng_q), a.reps)))
        rows.append(("index", median_ms(lambda: eng.pool_minimizer_index(rng_q), a.reps)))
    _, q = eng.pool_minimizers(rng_q)
    _, r_sorted, _, threshold = eng.pool_minimizer_index(rng_q)
    limit = np.array([max(1, s // 6) for s in range(4096)], np.int32)
    args = (q, r_sorted, int(threshold[0]), len(seq), a.init_len, 1, 1, limit)
    code, first, windows, out, used = eng.search_windows_raw(*args)
    assert code == 0
    cap = used + 16
    buf = np.zeros(cap, extz2.SEARCH_INTERVAL_DTYPE)
    if not a.kernels:
        rows.append(("host form", median_ms(lambda: eng.search_windows_raw(*args, cap=cap, out=buf), a.reps)))

    def up(x):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).cuda()
    d_q, d_r, d_limit = up(q), up(r_sorted), up(limit)
    d_first = torch.zeros(len(q) + 1, dtype=torch.int64, device="cuda")
    d_win = torch.zeros(len(q) * 20, dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(cap * 8, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def device_call():
        return eng.search_windows_device(d_q.data_ptr(), len(q), len(seq), d_r.data_ptr(), len(r_sorted), int(threshold[0]), a.init_len,
                                         1, 1, d_limit.data_ptr(), len(limit), d_first.data_ptr(), d_win.data_ptr(), d_out.data_ptr(), cap)
    if a.kernels:
        for _ in range(a.kernels):
            assert device_call() == used
        print("%d device-form calls on %d windows" % (a.kernels, len(q)))
        return
    rows.append(("device form", median_ms(device_call, a.reps)))
    rows.append(("host, 1 thread", median_ms(lambda: extz2.search_windows_host(*args, cap=cap, out=buf), a.reps)))
    ends = np.searchsorted(q["loc"], q["loc"].astype(np.int64) + a.init_len, "right")  # the member extent of every window
    cuts = np.linspace(0, len(q), a.threads + 1).astype(int)

    def share(t):
        lo, hi = int(cuts[t]), int(cuts[t + 1])
        if lo == hi:
            return 0
        sub = q[lo:int(ends[hi - 1])]
        code, f, w, o, u = extz2.search_windows_host(sub, *args[1:], cap=cap, out=np.zeros(cap, extz2.SEARCH_INTERVAL_DTYPE))
        assert code == 0
        return int(f[hi - lo])

    def threaded():
        with ThreadPoolExecutor(a.threads) as pool:
            return sum(pool.map(share, range(a.threads)))
    assert threaded() == used
    rows.append(("host, %d threads" % a.threads, median_ms(threaded, a.reps)))
    wide = int(((windows["flags"] & extz2.SEARCH_WIDE) != 0).sum())
    print("sequence %.2f Mb against itself, k 12, w 16, init_len %d: %d minimizers, %d intervals, threshold %d"
          % (len(seq) / 1e6, a.init_len, len(q), used, int(threshold[0])))
    print("windows: %d, WIDE %d (%.3f %%), with an interval %d; members mean %.1f max %d; gathered mean %.1f max %d"
          % (len(q), wide, 100.0 * wide / max(1, len(q)), int((np.diff(first.astype(np.int64)) > 0).sum()),
             windows["n_members"].mean(), windows["n_members"].max(), windows["n_gathered"].mean(), windows["n_gathered"].max()))
    for name, (med, lo, hi) in rows:
        print("%-18s median %10.2f ms   (min %.2f, max %.2f)" % (name, med, lo, hi))


if __name__ == "__main__":
    main()
