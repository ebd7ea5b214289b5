"""All-pairs search over eight records of 250 kb (the input of profiles/search_cmd.py, 64 pairs): the sequential loop of
sdf_search_pair_indexed -- one pair after the other on the owner, what `sedef search -t` does at SDF_SEARCH_LANES=1 -- against
one sdf_search_pairs_indexed call at 1, 2, 4, 8 and 16 lanes.  Per form: the hits (which must agree), the rounds summed over
the pairs, the median seconds of five calls after a warm-up, and sdf_device_bytes while the form's buffers are held.
A record, not a gate: it decides later whether SDF_SEARCH_LANES keeps its default of 1.  What the lanes assume is that a round
is bound by launch and wait latency, so that rounds of different pairs overlap; if the batch is no faster, that is what the
file says.  Every step's code is checked; the script stops at the first that is not 0.

    python profiles/search_lanes.py [--out FILE] [--records 8] [--bases 250000] [--repeats 5]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))


def step(code, what):
    if code != 0:
        sys.exit("%s: rc=%d" % (what, code))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_lanes.txt"))
    ap.add_argument("--records", type=int, default=8)
    ap.add_argument("--bases", type=int, default=250000)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import torch  # noqa: F401
    import sedef_amd
    from sedef_amd import extz2, host
    from search_cmd import genome
    recs = genome(a.records, a.bases)
    eng = sedef_amd.Extz2Engine(0)
    eng.pool_upload(b"".join(recs))
    eng.pool_sync()
    kw = dict(k=12, w=16, min_read_size=700, limit=host.limit_table(a.bases // 4))
    handles = []
    for i in range(a.records):
        code, h = eng.search_index_build((i * a.bases, a.bases, 0))
        step(code, "sdf_search_index_build %d" % i)
        handles.append(h)
    pairs = [(q, r) for r in range(a.records) for q in range(a.records)]  # (the command's order)
    lines = []

    def say(text):
        lines.append(text)
        print(text, flush=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    say("%d records of %d bases, %d pairs; median of %d calls after a warm-up" % (a.records, a.bases, len(pairs), a.repeats))

    def loop():
        hits, rounds = [], 0
        for q, r in pairs:
            same = q == r
            code, h, _, st = eng.search_pair_indexed(handles[q], handles[r], same_genome=same, extend=extz2.extend_params(same_genome=same), **kw)
            step(code, "sdf_search_pair_indexed (%d, %d)" % (q, r))
            hits.append(h.tobytes())
            rounds += int(st["rounds"])
        return hits, rounds

    def timed(call):
        call()  # (the warm-up pays for buffers and first launches)
        secs, last = [], None
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            last = call()
            secs.append(time.perf_counter() - t0)
        return statistics.median(secs), last

    t_loop, (want, rounds) = timed(loop)
    say("loop of sdf_search_pair_indexed:        %8.3f s  %d hits, %d rounds, %.1f MiB on the device" % (
        t_loop, sum(len(h) // 24 for h in want), rounds, eng.device_bytes() / 2.0**20))
    jobs = [(handles[q], handles[r], q == r) for q, r in pairs]
    for n in (1, 2, 4, 8, 16):
        code, lanes = eng.search_lanes_open(n)
        step(code, "sdf_search_lanes_open %d" % n)

        def batch():
            code, hits, first, stats = eng.search_pairs_indexed(lanes, jobs, **kw)
            step(code, "sdf_search_pairs_indexed on %d lanes" % n)
            return [hits[int(first[j]):int(first[j + 1])].tobytes() for j in range(len(jobs))], sum(int(s["rounds"]) for s in stats)

        t, (got, got_rounds) = timed(batch)
        if got != want:
            sys.exit("%d lanes: the hits differ from the loop's" % n)
        say("sdf_search_pairs_indexed, %2d lanes:      %8.3f s  %d hits, %d rounds, %.1f MiB on the device (%.2f x the loop)" % (
            n, t, sum(len(h) // 24 for h in got), got_rounds, eng.device_bytes() / 2.0**20, t_loop / t))
        step(eng.search_lanes_close(lanes), "sdf_search_lanes_close")
    eng.close()


if __name__ == "__main__":
    main()
