#!/usr/bin/env python3
"""CPU: the time of the search family's host forms in two builds of the library, alternating, a fresh process per run.
usage: search_host.py parent/libsedef_hip.so branch/libsedef_hip.so [runs=5]        (writes profiles/search_host.txt's table to stdout)
Cases: sdf_search_roll_host on every case of tests/golden/search_roll_kat.json.gz, sdf_search_extend_host on every case of
tests/golden/search_extend_long_kat.json.gz, sdf_search_pair_host on the three drawn pairs of tests/test_search_driver_cpu.py.
A run's figure is the sum over the cases of the time around the ctypes call alone (REPEAT calls each), in milliseconds."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPEAT = 5
NAMES = ("sdf_search_roll_host", "sdf_search_extend_host", "sdf_search_pair_host")


def child(lib_path):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from sedef_amd import extz2
    extz2.LIB_PATH = lib_path
    lib = extz2.load_library()
    spent = dict.fromkeys(NAMES, 0.0)

    def timed(name):
        f = getattr(lib, name)

        def call(*args):
            t0 = time.perf_counter()
            rc = f(*args)
            spent[name] += time.perf_counter() - t0
            return rc
        setattr(lib, name, call)

    import test_search_driver_cpu as TD
    import test_search_extend_cpu as TE
    import test_search_extend_long_cpu as TL
    import test_search_roll_cpu as TR
    rolls = [TR.case_inputs(c) for c in TR.load_fixture()["cases"]]
    longs = [TE.case_extend_inputs(c) for c in TL.load_fixture()["cases"]]
    pairs = [TD.DM.inputs(*which) for which in TD.INPUTS]
    for name in NAMES:
        timed(name)
    for _ in range(REPEAT):
        for args in rolls:
            assert TR.host(*args)[0] == 0
        for args, params in longs:
            assert TE.host(args, params)[0] == 0
        for I in pairs:
            assert TD.host_pair(I)[0] == 0
    print(json.dumps({k: 1e3 * v for k, v in spent.items()}))


def main():
    libs = {"parent": os.path.abspath(sys.argv[1]), "branch": os.path.abspath(sys.argv[2])}
    runs = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    series = {who: {n: [] for n in NAMES} for who in libs}
    for _ in range(runs):
        for who, path in libs.items():
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path], check=True, stdout=subprocess.PIPE, text=True)
            for n, ms in json.loads(out.stdout.strip().splitlines()[-1]).items():
                series[who][n].append(ms)
    print("ms per run (%d calls of every case), %d runs each, alternating; median [min .. max]" % (REPEAT, runs))
    for n in NAMES:
        for who in libs:
            s = series[who][n]
            print("%-24s %-6s %9.2f [%9.2f .. %9.2f]" % (n, who, statistics.median(s), min(s), max(s)))
        ok = statistics.median(series["branch"][n]) <= max(series["parent"][n])
        print("%-24s branch median %s the parent's slowest run" % (n, "at or below" if ok else "ABOVE"))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        main()
