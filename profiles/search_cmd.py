"""All-pairs search over eight records of 250 kb, as `sedef search -t` loops: once through sdf_search_pair per pair (both
ranges' minimizers and the reference's index in every call) and once through resident handles (sdf_search_index_build per
record, sdf_search_pair_indexed per pair).  Prints wall times, the hits of both (which must agree) and the indexes built.
A record of one run, not a gate: profiles/search_cmd.txt holds what it printed on the MI355X.

    python profiles/search_cmd.py [records] [bases]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def genome(n_rec, n_bases, seed=1):
    """Random records; every record but the first carries two copies of 3 kb from the record before it at 5 % substitutions."""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGT", np.uint8)
    recs = [letters[rng.integers(0, 4, n_bases)].copy() for _ in range(n_rec)]
    for i in range(1, n_rec):
        for j in range(2):
            src = int(rng.integers(0, n_bases - 3000))
            dst = int(rng.integers(0, n_bases - 3000))
            piece = recs[i - 1][src:src + 3000].copy()
            flip = rng.random(3000) < 0.05
            piece[flip] = letters[rng.integers(0, 4, int(flip.sum()))]
            recs[i][dst:dst + 3000] = piece
    return [r.tobytes() for r in recs]


def main():
    import torch  # noqa: F401
    import sedef_amd
    from sedef_amd import extz2, host
    n_rec = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    n_bases = int(sys.argv[2]) if len(sys.argv) > 2 else 250000
    recs = genome(n_rec, n_bases)
    eng = sedef_amd.Extz2Engine(0)
    eng.pool_upload(b"".join(recs))
    eng.pool_sync()
    ranges = [(i * n_bases, n_bases, 0) for i in range(n_rec)]
    t0 = time.perf_counter()
    limit = host.limit_table(n_bases // 4)
    t_limit = time.perf_counter() - t0
    kw = dict(k=12, w=16, min_read_size=700, limit=limit)

    def params(q, r):
        same = q == r
        return dict(kw, same_genome=same, extend=extz2.extend_params(same_genome=same))
    for warm in (True, False):  # (the first pass pays for buffers and first launches)
        t0 = time.perf_counter()
        per_call = [eng.search_pair(ranges[q], ranges[r], **params(q, r)) for r in range(n_rec) for q in range(n_rec)]
        t_calls = time.perf_counter() - t0
        b0 = eng.search_index_builds()[0]
        t0 = time.perf_counter()
        handles = [eng.search_index_build(rg)[1] for rg in ranges]
        t_build = time.perf_counter() - t0
        indexed = [eng.search_pair_indexed(handles[q], handles[r], **params(q, r)) for r in range(n_rec) for q in range(n_rec)]
        t_indexed = time.perf_counter() - t0
        built = eng.search_index_builds()[0] - b0
        for h in handles:
            eng.search_index_free(h)
        assert all(a[0] == 0 and b[0] == 0 and a[1].tobytes() == b[1].tobytes() for a, b in zip(per_call, indexed))
        if not warm:
            print("%d records of %d bases, %d pairs, %d hits; limit table of %d entries in %.2f s" % (
                n_rec, n_bases, n_rec * n_rec, sum(a[2] for a in indexed), len(limit) - 1, t_limit))
            print("sdf_search_pair per pair:          %.3f s (%d index computations)" % (t_calls, 2 * n_rec * n_rec))
            print("handles + sdf_search_pair_indexed: %.3f s (%d indexes built in %.3f s)" % (t_indexed, built, t_build))
    eng.close()


if __name__ == "__main__":
    main()
