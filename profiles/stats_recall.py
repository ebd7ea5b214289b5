"""Pair recall: sdf_pair_recall_host, sdf_pair_recall and sdf_pair_recall_device once each, in one process, on a synthetic set of
the size `sedef stats recall` meets -- a WGAC-sized gold list against a final.bed-sized found list, generated here.  Most
records lie alone; a share of both sets crowds around a few hundred places, the first of them the densest, so that some gold records
collect hundreds of hits and a few more than the LDS lists hold.  Per form: a warm-up call, then the seconds of one call (a host clock around a call that
has returned; the `_device` form is followed by a wait on the context's stream and times neither the uploads nor the copy back).
The comparison that matters is the device call against sdf_pair_recall_host on the same input in the same session; the share of
gold records that took the WIDE path is reported with it.  A record, not a gate: nobody fixed a ratio in advance.

    python profiles/stats_recall.py [--out FILE] [--gold 50000] [--found 400000] [--places 300]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def records(rng, n, places, crowded, rc):
    """n records on 24 chromosomes of 150 Mb; `crowded` of them within 20 kb of one of the places (pairs of loci)"""
    r = np.zeros(n, rc.PAIR_REC_DTYPE)
    r["chr1"], r["chr2"] = rng.integers(0, 24, n), rng.integers(0, 24, n)
    r["start1"], r["start2"] = rng.integers(0, 150 * 10 ** 6, n), rng.integers(0, 150 * 10 ** 6, n)
    at = rng.permutation(n)[:int(crowded * n)]
    p = places[(rng.random(len(at)) ** 1.3 * len(places)).astype(np.int64)]  # (the first places are the densest)
    r["chr1"][at], r["chr2"][at] = p[:, 0], p[:, 2]
    r["start1"][at], r["start2"][at] = p[:, 1] + rng.integers(0, 20000, len(at)), p[:, 3] + rng.integers(0, 20000, len(at))
    r["end1"], r["end2"] = r["start1"] + rng.integers(1000, 30000, n), r["start2"] + rng.integers(1000, 30000, n)
    r["flags"] = rng.integers(0, 4, n) * (rng.random(n) < 0.2)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stats_recall.txt"))
    ap.add_argument("--gold", type=int, default=50000)
    ap.add_argument("--found", type=int, default=400000)
    ap.add_argument("--places", type=int, default=300)
    a = ap.parse_args()
    import torch
    import sedef_amd
    from sedef_amd import recall as rc
    rng = np.random.default_rng(2026)
    places = np.stack([rng.integers(0, 24, a.places), rng.integers(0, 150 * 10 ** 6, a.places), rng.integers(0, 24, a.places),
                       rng.integers(0, 150 * 10 ** 6, a.places)], axis=1)
    gold, found = records(rng, a.gold, places, 0.3, rc), records(rng, a.found, places, 0.3, rc)
    eng = sedef_amd.Extz2Engine(0)
    lines = []

    def say(text):
        lines.append(text)
        print(text, flush=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    def up(x):
        return torch.from_numpy(x.view(np.uint8).reshape(-1).copy()).cuda()
    d_gold, d_found = up(gold), up(found)
    d_out = torch.zeros(len(gold) * 16, dtype=torch.uint8, device="cuda")
    d_status = torch.zeros(2, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    def device_call():
        rc.pair_recall_device(eng, d_gold.data_ptr(), len(gold), d_found.data_ptr(), len(found), 0, d_out.data_ptr(), d_status.data_ptr())
        eng.pool_sync()

    forms = {"sdf_pair_recall_host": lambda: rc.pair_recall_host(gold, found, 0)[1],
             "sdf_pair_recall": lambda: rc.pair_recall(eng, gold, found, 0),
             "sdf_pair_recall_device": device_call}
    say("pair recall (profiles/stats_recall.py): %d gold against %d found records, 30%% of each around %d places; GPU_MAX_HW_QUEUES=%s"
        % (len(gold), len(found), a.places, os.environ.get("GPU_MAX_HW_QUEUES", "unset")))
    want = forms["sdf_pair_recall_host"]()  # (warm-up of the host form, and the answer)
    assert forms["sdf_pair_recall"]().tobytes() == want.tobytes()
    device_call()
    dev = d_out.cpu().numpy().view(rc.RECALL_DTYPE)
    wide = (want["flags"] & rc.WIDE) != 0
    assert (dev["n_hits"] == want["n_hits"]).all() and (dev["flags"] == want["flags"]).all() and dev[~wide].tobytes() == want[~wide].tobytes()
    say("gold records hit: %d; most hits on one: %d; with 100 hits or more: %d; WIDE (more than %d list entries): %d = %.3f%% of the gold records"
        % (int((want["n_hits"] > 0).sum()), int(want["n_hits"].max()), int((want["n_hits"] >= 100).sum()), rc.CAP, int(wide.sum()),
           100.0 * wide.sum() / len(gold)))
    secs = {}
    for name, f in forms.items():
        t0 = time.perf_counter()
        f()
        secs[name] = time.perf_counter() - t0
        say("%-24s %.4f s" % (name, secs[name]))
    say("sdf_pair_recall_host / sdf_pair_recall_device: %.1f; / sdf_pair_recall (uploads, copy back and the WIDE records on the host included): %.1f"
        % (secs["sdf_pair_recall_host"] / secs["sdf_pair_recall_device"], secs["sdf_pair_recall_host"] / secs["sdf_pair_recall"]))


if __name__ == "__main__":
    main()
