"""`stats diff`'s one device call against its host form: sdf_pool_coverage and sdf_pool_coverage_host in the same process, on eight
records of 250,000 bases with 20,000 intervals of 1-100 kb -- half of them pairs of set 0 that are partners of each other (a
final.bed), half single intervals of set 1 (a WGAC table).  Per form: the median seconds of five calls after a warm-up (a host
clock around a call that returns behind a stream synchronise), the two alternating so that both see the same machine; the
results must agree.  The device call's time includes its uploads of the records and its copies back, not the chromosomes'
upload.  A record, not a gate: nobody fixed a ratio in advance.  The queue setting of the run is written with the figures.

    python profiles/stats_diff.py [--out FILE] [--records 8] [--bases 250000] [--intervals 20000] [--repeats 5]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stats_diff.txt"))
    ap.add_argument("--records", type=int, default=8)
    ap.add_argument("--bases", type=int, default=250000)
    ap.add_argument("--intervals", type=int, default=20000)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import torch  # noqa: F401
    import sedef_amd
    from sedef_amd import extz2
    rng = np.random.default_rng(2025)
    # soft-masked bases: a third lowercase in stretches of a few hundred, an N run per record
    recs = []
    for _ in range(a.records):
        s = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, a.bases)].copy()
        for at in rng.integers(0, a.bases, a.bases // 900):
            s[at:at + 300] |= 0x20
        at = int(rng.integers(0, a.bases - 2000))
        s[at:at + 1000] = ord("N")
        recs.append(s)
    chars = np.concatenate(recs).tobytes()
    regions = [(r * a.bases, a.bases) for r in range(a.records)]
    iv = np.zeros(a.intervals, extz2.COVER_INTERVAL_DTYPE)
    iv["region"] = rng.integers(0, a.records, a.intervals)
    iv["len"] = rng.integers(1000, min(100000, a.bases) + 1, a.intervals)
    iv["start"] = (rng.random(a.intervals) * (a.bases - iv["len"] + 1)).astype(np.int64)
    half = a.intervals // 2 // 2 * 2
    iv["set"][half:] = 1
    iv["partner"] = -1
    iv["partner"][:half] = np.arange(half) ^ 1
    eng = sedef_amd.Extz2Engine(0)
    eng.pool_upload(chars)
    eng.pool_sync()
    lines = []

    def say(text):
        lines.append(text)
        print(text, flush=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    say("%d records of %d bases, %d intervals of 1-100 kb (%d bases painted over); median of %d calls after a warm-up, the forms alternating" % (
        a.records, a.bases, a.intervals, int(iv["len"].sum()), a.repeats))
    say("GPU_MAX_HW_QUEUES=%s" % os.environ.get("GPU_MAX_HW_QUEUES", "(unset: the runtime's default)"))

    def device():
        return eng.pool_coverage(regions, iv, 100)

    def on_host():
        rc, out = extz2.pool_coverage_host(chars, regions, iv, 100)
        if rc != 0:
            sys.exit("sdf_pool_coverage_host: rc=%d" % rc)
        return out

    got, want = device(), on_host()  # (the warm-up pays for buffers and first launches)
    secs = {"device": [], "host": []}
    for _ in range(a.repeats):
        for name, call in (("device", device), ("host", on_host)):
            t0 = time.perf_counter()
            out = call()
            secs[name].append(time.perf_counter() - t0)
            if name == "device":
                got = out
    for x, y in zip(got, want):
        if x.tobytes() != y.tobytes():
            sys.exit("the device's results differ from the host form's")
    t_dev, t_host = statistics.median(secs["device"]), statistics.median(secs["host"])
    say("sdf_pool_coverage:       %9.5f s  (min %.5f, max %.5f; %.1f MiB on the device, the pool included)" % (
        t_dev, min(secs["device"]), max(secs["device"]), eng.device_bytes() / 2.0**20))
    say("sdf_pool_coverage_host:  %9.5f s  (min %.5f, max %.5f)  %.1f x the device call" % (t_host, min(secs["host"]), max(secs["host"]), t_host / t_dev))
    say("painted %d of %d intervals; a = %d, b = %d, both = %d over all regions" % (
        int(got[2].sum()), a.intervals, int(got[0]["a"].sum()), int(got[0]["b"].sum()), int(got[0]["both"].sum())))
    eng.close()


if __name__ == "__main__":
    main()
