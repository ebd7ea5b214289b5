"""Throughput of the stats columns kernels on synthetic SD-shaped alignments resident in HBM.
python profiles/stats_probe.py [n_alignments] [mean_len] [--resident] [--rc-frac F] [--repeats R]
  -> ms per launch (HIP events around the launches) and GB/s of algorithmic bytes (a_len + b_len + 4 n_cigar + 64).
default        sdf_stats_columns_device on a pool of the caller's own;
--resident     sdf_stats_columns_pairs_device on the context's resident pool (sdf_pool_upload);
--rc-frac F    with --resident: a fraction F of the sides carries a strand bit (0: forward tasks, any_rc = 0);
--repeats R    R timed repeats of twenty launches each: one line per repeat, then min / median / max."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sedef_amd  # noqa: E402
from sedef_amd.extz2 import STATS_COLS_DTYPE, STATS_TASK_DTYPE  # noqa: E402


def build(n, mean_len, seed=1):
    rng = np.random.default_rng(seed)
    lens = np.maximum(200, rng.exponential(mean_len, n)).astype(np.int64)
    # run structure of a ~10 % divergent alignment: M runs of ~40 columns, a short gap between them
    tasks = np.zeros(n, STATS_TASK_DTYPE)
    cig_parts, off, coff = [], 0, 0
    for k in range(n):
        nrun = max(1, int(lens[k] // 45))
        m = rng.integers(1, 80, nrun).astype(np.uint32)
        g = rng.integers(1, 6, nrun).astype(np.uint32)
        op = rng.integers(1, 3, nrun).astype(np.uint32)
        cg = np.empty(2 * nrun, np.uint32)
        cg[0::2] = m << 4
        cg[1::2] = (g << 4) | op
        na = int(m.sum() + g[op == 1].sum())
        nb = int(m.sum() + g[op == 2].sum())
        tasks[k] = (off, off + na, na, nb, coff, len(cg), 0)
        off += na + nb
        coff += len(cg)
        cig_parts.append(cg)
    pool = rng.choice(np.frombuffer(b"ACGTacgt", np.uint8), off)
    return tasks, pool, np.concatenate(cig_parts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", nargs="?", type=int, default=20000)
    ap.add_argument("mean_len", nargs="?", type=int, default=10000)
    ap.add_argument("--resident", action="store_true")
    ap.add_argument("--rc-frac", type=float, default=0.0)
    ap.add_argument("--repeats", type=int, default=1)
    a = ap.parse_args()
    if a.rc_frac and not a.resident:
        ap.error("--rc-frac needs --resident: only the calls on the resident pool read strand bits")
    n = a.n
    tasks, pool, cig = build(n, a.mean_len)
    if a.rc_frac:  # strand bits on a fraction of the SIDES, drawn per side
        rng = np.random.default_rng(2)
        tasks["reserved"] = (rng.random(n) < a.rc_frac) * sedef_amd.extz2.STATS_A_RC + \
            (rng.random(n) < a.rc_frac) * sedef_amd.extz2.STATS_B_RC
    eng = sedef_amd.Extz2Engine(0)
    dev = torch.device("cuda:0")
    d_tasks = torch.from_numpy(tasks.view(np.uint8)).to(dev)
    d_cig = torch.from_numpy(cig.view(np.int32)).to(dev)
    d_out = torch.zeros(n * 64, dtype=torch.uint8, device=dev)
    if a.resident:
        eng.pool_upload(pool.tobytes())
        eng.pool_sync()
        any_rc = int(a.rc_frac > 0)

        def launch(stream):
            eng.stats_columns_pairs_device(d_tasks.data_ptr(), n, any_rc, d_cig.data_ptr(), d_out.data_ptr(), stream)
        what = "sdf_stats_columns_pairs_device, %.0f %% of the sides reversed" % (100 * a.rc_frac)
    else:
        d_pool = torch.from_numpy(pool).to(dev)

        def launch(stream):
            eng.stats_columns_device(d_tasks.data_ptr(), n, d_pool.data_ptr(), d_cig.data_ptr(), d_out.data_ptr(), stream)
        what = "sdf_stats_columns_device"
    bytes_alg = int(tasks["a_len"].sum() + tasks["b_len"].sum()) + 4 * len(cig) + 64 * n
    st = torch.cuda.Stream()
    reps, times = 20, []
    with torch.cuda.stream(st):
        for _ in range(3):
            launch(st.cuda_stream)
        for _ in range(a.repeats):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record(st)
            for _ in range(reps):
                launch(st.cuda_stream)
            ev[1].record(st)
            st.synchronize()
            times.append(ev[0].elapsed_time(ev[1]) / reps)
    out = d_out.cpu().numpy().view(STATS_COLS_DTYPE)
    cols = int(out["span"].astype(np.int64).sum())
    assert int(out["flags"].sum()) == 0
    print("# %s" % what)
    for ms in times:
        print("stats columns: %d alignments, %.1f M columns, %.1f MB algorithmic: %.3f ms per launch = %.0f GB/s "
              "(%.3f of 8 TB/s), %.1f Gcolumn/s" % (n, cols / 1e6, bytes_alg / 1e6, ms, bytes_alg / ms / 1e6,
                                                  bytes_alg / ms / 1e6 / 8000, cols / ms / 1e6))
    if len(times) > 1:
        print("ms per launch over %d repeats: min %.3f median %.3f max %.3f; checksum %d" %
              (len(times), min(times), float(np.median(times)), max(times), int(out["match_b"].astype(np.int64).sum())))


if __name__ == "__main__":
    main()
