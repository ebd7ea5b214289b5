#!/usr/bin/env python3
"""Planning time on the CPU, two builds of the library against each other: cut_batch + plan_chunk through the
sdf_debug_plan_dump hook (its own timer: the cut and the chunk planning, not the digests), for the 100,000-task headline
batch, the 420,000-task batch (on threads: the cut in two passes, early start) and the 40,000-task mm8-like batch of
tests/golden/make_golden_plans.py, on 0 and 3 planning threads.  The builds alternate, a fresh process per run (one warm-up
plan, then the median of five per batch); prints every run and, per (batch, threads), both medians and the first build's
slowest run.
usage: plan_time.py PARENT.so BRANCH.so [RUNS]        (internal: plan_time.py --one LIB.so)"""
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests", "golden"))


def one(path):
    import make_golden_plans as g
    lib = g.load(path)
    out = {}
    for name, build, env in (("headline_100k", g.headline, {}), ("two_pass_420k", g.two_pass, {"SDF_DEBUG_PLAN_EARLY": 1}),
                             ("mm8_40k", g.mm8_40k, {})):
        t = build()
        for threads in g.THREADS:
            ms = []
            for _ in range(6):
                g.plan_digest(lib, t, threads, env=env if threads else {}, ms=ms)
            out["%s|t%d" % (name, threads)] = statistics.median(ms[1:])
    print(json.dumps(out))


def main():
    if sys.argv[1] == "--one":
        return one(sys.argv[2])
    libs = sys.argv[1:3]
    runs = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    series = [{}, {}]
    for r in range(runs):
        for i, lib in enumerate(libs):
            got = json.loads(subprocess.check_output([sys.executable, os.path.abspath(__file__), "--one", lib]).decode().splitlines()[-1])
            for k, v in got.items():
                series[i].setdefault(k, []).append(v)
    for k in series[0]:
        a, b = series[0][k], series[1][k]
        print("%-18s parent ms %s\n%-18s branch ms %s" % (k, " ".join("%.3f" % x for x in a), "", " ".join("%.3f" % x for x in b)))
        print("%-18s parent median %.3f slowest %.3f | branch median %.3f -> %s" %
              ("", statistics.median(a), max(a), statistics.median(b), "ok" if statistics.median(b) <= max(a) else "SLOWER"))


if __name__ == "__main__":
    main()
