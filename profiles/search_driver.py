#!/usr/bin/env python3
"""Times the search driver on a drawn pair with SD-like repeats: sdf_search_pair at a sweep of round sizes and at the default,
sdf_search_pair_host on one thread, and the share of kernel time per stage from one `rocprofv3 --kernel-trace --stats` run of
this script's own (--child: the run that is traced).  Writes profiles/search_driver.txt.

usage: search_driver.py [--bases 2000000] [--host-bases 200000] [--sweep 16,64,256,1024] [--no-trace]
The host form scans the whole found list per interval; it is timed on the first --host-bases of each sequence."""
import argparse
import csv
import glob
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LETTERS = np.frombuffer(b"ACGT", np.uint8)
STAGES = (("windows", ("search_keys", "search_prev", "search_lookup", "search_window", "stats_cuts_scan", "found_")),
          ("roll", ("search_roll",)), ("filter", ("search_filter",)), ("overlap", ("search_overlap",)),
          ("extend", ("search_extend_kernel", "search_hit_tasks")), ("extend long", ("search_extend_long",)),
          ("accept", ("search_accept",)), ("minimizers", ("minim_",)))


def draw(rng, bases, unit_len=3000, every=40000):
    """Random bases with a mutated copy of one of eight repeat units about every `every` bases."""
    units = [rng.integers(0, 4, unit_len) for _ in range(8)]
    parts, n = [], 0
    while n < bases:
        gap = rng.integers(0, 4, int(rng.integers(every // 2, every)))
        u = units[int(rng.integers(0, len(units)))].copy()
        hit = rng.random(len(u)) < 0.05
        u[hit] = (u[hit] + 1) % 4
        parts += [gap, u]
        n += len(gap) + len(u)
    return LETTERS[np.concatenate(parts)[:bases]].tobytes()


def limit_table(n=4096, k=12, max_error=0.30):
    """A stand-in for the caller's table of relaxed_jaccard_estimate(s) (src/util.cc:85, which needs Boost's binomial quantile):
    half of s * tau(max_error, k), at least 1.  The table decides how many intervals a window has, so the figures hold for it."""
    tau = 1.0 / (2.0 * np.exp(k * max_error) - 1.0)
    return [max(1, int(s * tau * 0.5)) for s in range(n)]


def run(eng, extz2, qs, rs, **kw):
    eng.pool_upload(qs + rs)
    eng.pool_sync()
    t = time.perf_counter()
    rc, hits, used, stats = eng.search_pair((0, len(qs), 0), (len(qs), len(rs), 0), limit=limit_table(), **kw)
    assert rc == 0, rc
    return time.perf_counter() - t, len(hits), {f: int(stats[f]) for f in stats.dtype.names}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=int, default=2000000)
    ap.add_argument("--host-bases", type=int, default=200000)
    ap.add_argument("--sweep", default="16,64,256,1024")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    import sedef_amd
    from sedef_amd import extz2
    rng = np.random.default_rng(1)
    qs, rs = draw(rng, a.bases), draw(rng, a.bases)
    eng = sedef_amd.Extz2Engine(0)
    run(eng, extz2, qs[:100000], rs[:100000])  # warm-up: buffers, code objects
    if a.child:
        run(eng, extz2, qs, rs)
        return
    lines = ["search driver on a drawn pair of 2 x %d bases (profiles/search_driver.py)" % a.bases]
    for rw in [int(x) for x in a.sweep.split(",")] + [0]:
        sec, n, st = run(eng, extz2, qs, rs, round_windows=rw)
        lines.append("round_windows %5s: %8.3f s  hits %d  rounds %d  windows run %d of %d scheduled  host %d  rounds per hit %.3f"
                     % (rw or "dflt", sec, n, st["rounds"], st["windows_run"], st["windows_scheduled"], st["windows_host"], st["rounds"] / max(1, n)))
    hq, hr = qs[:a.host_bases], rs[:a.host_bases]
    t = time.perf_counter()
    rc, hits, used, st = extz2.search_pair_host(hq + hr, (0, len(hq), 0), (len(hq), len(hr), 0), limit=limit_table())
    lines.append("sdf_search_pair_host, one thread, 2 x %d bases: %8.3f s  hits %d" % (a.host_bases, time.perf_counter() - t, len(hits)))
    sec, n, st = run(eng, extz2, hq, hr)
    lines.append("sdf_search_pair on the same: %8.3f s  hits %d" % (sec, n))
    if not a.no_trace:
        with tempfile.TemporaryDirectory() as d:
            subprocess.check_call(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
                                   os.path.abspath(__file__), "--child", "--bases", str(a.bases)])
            total, per = 0.0, {name: 0.0 for name, _ in STAGES}
            for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
                for row in csv.DictReader(open(path)):
                    ns = float(row.get("TotalDurationNs") or 0)
                    total += ns
                    for name, keys in STAGES:
                        if any(k in row["Name"] for k in keys):
                            per[name] += ns
                            break
            lines.append("kernel time per stage (one traced run at the default round size): " +
                         ", ".join("%s %.1f%%" % (name, 100 * ns / max(total, 1)) for name, ns in per.items()))
    open(os.path.join(ROOT, "profiles", "search_driver.txt"), "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
