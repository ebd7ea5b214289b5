"""`align bucket` on records: sdf_bucket_merge_host, sdf_bucket_merge and sdf_bucket_merge_device in one process, on 2,000,000
synthetic seed hits of six chromosomes in three groups -- about a tenth of them in 50 dense runs of 4,000 hits each (a
repeat-dense region: query starts a few bases apart, reference places all over), the rest spread so that most runs hold one or
two hits.  Per form: a warm-up call, then the seconds of every one of `--repeats` calls (a host clock around a call that has
returned; the `_device` form is followed by a wait on the context's stream and times neither the uploads nor the copy back) and
their range; the forms alternate so that all see the same machine; the records must agree.  The longest run's sweep alone: the
`_device` form on the 4,000 hits of ONE dense run (a call of nine launches, of which the sweep is the only one whose time grows
with the square of the run).  A record, not a gate: nobody fixed a ratio in advance.

    python profiles/bucket_merge.py [--out FILE] [--hits 2000000] [--runs 50] [--run-hits 4000] [--repeats 5]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def seeds(rng, n, runs, run_hits, bk):
    h = np.zeros(n, bk.SEED_HIT_DTYPE)
    h["q_chr"], h["r_chr"] = rng.integers(0, 6, n), rng.integers(0, 6, n)
    h["q_start"], h["r_start"] = rng.integers(0, 200 * 10 ** 6, n), rng.integers(0, 200 * 10 ** 6, n)
    h["q_end"], h["r_end"] = h["q_start"] + rng.integers(700, 3000, n), h["r_start"] + rng.integers(700, 3000, n)
    h["flags"] = rng.random(n) < 0.3
    for r in range(runs):  # a dense run: one pair of chromosomes, query starts 5 apart, 400 places in 40 Mb of the reference
        at = slice(r * run_hits, (r + 1) * run_hits)
        h["q_chr"][at], h["r_chr"][at], h["flags"][at] = r % 6, (r // 6) % 6, 0
        h["q_start"][at] = 10 ** 6 * (r + 1) + 5 * np.arange(run_hits)
        h["q_end"][at] = h["q_start"][at] + 1000
        h["r_start"][at] = 10 ** 5 * rng.integers(0, 400, run_hits) + rng.integers(0, 2000, run_hits)
        h["r_end"][at] = h["r_start"][at] + 1000
    return h[rng.permutation(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bucket_merge.txt"))
    ap.add_argument("--hits", type=int, default=2000000)
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--run-hits", type=int, default=4000)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import torch
    import sedef_amd
    from sedef_amd import bucket as bk
    rng = np.random.default_rng(2026)
    hits = seeds(rng, a.hits, a.runs, a.run_hits, bk)
    chr_group, order, P = np.array([0, 1, 2, 1, 0, 2], np.int32), bk.pair_order(3), bk.bucket_params(64)
    eng = sedef_amd.Extz2Engine(0)
    lines = []

    def say(text):
        lines.append(text)
        print(text, flush=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    def up(x):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).cuda()

    def device_call(h):
        d_hits, d_grp, d_ord = up(h), up(chr_group), up(order)
        d_out = torch.zeros(len(h) * 32, dtype=torch.uint8, device="cuda")
        d_n = torch.zeros(2, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()

        def call():
            bk.bucket_merge_device(eng, d_hits.data_ptr(), len(h), d_grp.data_ptr(), 6, d_ord.data_ptr(), 3, P, d_out.data_ptr(), len(h), d_n.data_ptr())
            eng.pool_sync()
            return d_out[:int(d_n[0]) * 32].cpu().numpy().view(bk.BUCKET_HIT_DTYPE)
        return call

    forms = {"sdf_bucket_merge_host": lambda: bk.bucket_merge_host(hits, chr_group, order, P)[1],
             "sdf_bucket_merge": lambda: bk.bucket_merge(eng, hits, chr_group, order, P),
             "sdf_bucket_merge_device": device_call(hits)}
    say("align bucket on records: %d seed hits, %d dense runs of %d; GPU_MAX_HW_QUEUES=%s" % (a.hits, a.runs, a.run_hits,
                                                                                            os.environ.get("GPU_MAX_HW_QUEUES", "unset")))
    want = forms["sdf_bucket_merge_host"]()  # (warm-up of the host form, and the answer)
    for name in ("sdf_bucket_merge", "sdf_bucket_merge_device"):
        got = forms[name]()  # (warm-up: buffers, hipCUB)
        assert got.tobytes() == want.tobytes(), name
    say("records out: %d, equal in the three forms" % len(want))
    secs = {name: [] for name in forms}
    for _ in range(a.repeats):
        for name, f in forms.items():
            t0 = time.perf_counter()
            f()
            secs[name].append(time.perf_counter() - t0)
    for name, s in secs.items():
        say("%-26s %s s  (range %.4f - %.4f)" % (name, " ".join("%.4f" % x for x in s), min(s), max(s)))
    one = hits[(hits["q_start"] >= 10 ** 6) & (hits["q_start"] < 10 ** 6 + 5 * a.run_hits) & (hits["q_chr"] == 0) & (hits["r_chr"] == 0) & (hits["q_end"] - hits["q_start"] == 1000)]
    call = device_call(one)
    call()
    s = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        call()
        s.append(time.perf_counter() - t0)
    say("one dense run alone (%d hits, _device form; the sweep of one wavefront): %s s  (range %.4f - %.4f)" % (len(one), " ".join("%.4f" % x for x in s),
                                                                                                                  min(s), max(s)))


if __name__ == "__main__":
    main()
