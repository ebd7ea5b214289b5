#!/usr/bin/env python3
"""sdf_search_pair against sdf_search_pair_wide on a pair whose scheduled windows are WIDE for the seeding kernel alone: the
seed-WIDE pair of tests/wide_model.py (a unit of 100 bases, about a hundred copies in the reference) with a query array long
enough for a few hundred scheduled windows.  Wall clock of the whole call, same process, one warm-up and the median of five
runs each; rounds and windows_host of both.  Writes profiles/search_wide.txt (the kernels' resource figures stay at its top).
usage: search_wide.py [q_copies] [n_wide_max]"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402,F401  (before the library brings a HIP runtime of its own along)

import driver_model as DM  # noqa: E402
import wide_model as WM  # noqa: E402

HEAD = """search_seeds_wide.hip (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage)
  search_window_wide_kernel<false, false>  25 VGPRs, 45 SGPRs, LDS 135,248 B, scratch 0, no spills, 1 workgroup / CU
  search_window_wide_kernel<true,  false>  26 VGPRs, 51 SGPRs, LDS 135,248 B, scratch 0, no spills
  search_window_wide_kernel<false, true>   31 VGPRs, 86 SGPRs, LDS 139,344 B, scratch 0, no spills
  search_window_wide_kernel<true,  true>   31 VGPRs, 88 SGPRs, LDS 139,344 B, scratch 0, no spills
  search_wide_list_kernel                  41 VGPRs, 59 SGPRs, LDS 64 B, scratch 0
profiles/isa_same.py parent / branch: 1185 functions in both, 1185 identical; only in branch: the five kernels above
"""


def main():
    import sedef_amd
    from sedef_amd import extz2
    q_copies = int(sys.argv[1]) if len(sys.argv) > 1 else 120
    n_wide = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    I = WM.wide_pair(q_copies=q_copies)
    kw = DM.pair_kwargs(extz2, I)
    eng = sedef_amd.Extz2Engine(0)
    eng.pool_upload(I["pool"])
    eng.pool_sync()
    lines = []
    answers = {}
    for name, call in (("sdf_search_pair", lambda: eng.search_pair(I["q_range"], I["r_range"], **kw)),
                       ("sdf_search_pair_wide(%d)" % n_wide, lambda: eng.search_pair_wide(I["q_range"], I["r_range"], n_wide_max=n_wide, **kw))):
        call()  # warm-up
        times = []
        for _ in range(5):
            t0 = time.perf_counter()
            rc, hits, used, stats = call()
            times.append(time.perf_counter() - t0)
            assert rc == 0
        answers[name] = hits.tobytes()
        lines.append("%-26s median %8.2f ms  (min %.2f, max %.2f)  hits %d  scheduled %d  rounds %d  windows_run %d  windows_host %d" % (
            name, 1e3 * statistics.median(times), 1e3 * min(times), 1e3 * max(times), used, int(stats["windows_scheduled"]),
            int(stats["rounds"]), int(stats["windows_run"]), int(stats["windows_host"])))
    assert len(set(answers.values())) == 1, "the two forms disagree"
    eng.close()
    text = HEAD + "\nquery array of %d copies, reference of 100, init_len %d, round_windows default; wall clock per call, median of 5 after a warm-up\n" % (
        q_copies, I["init_len"]) + "\n".join(lines) + "\n"
    print(text)
    with open(os.path.join(ROOT, "profiles", "search_wide.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
