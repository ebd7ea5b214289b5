"""The seeding phase of sedef.sh both ways on one generated genome, once each: the old way -- one `sedef search [-r] -t i j`
process per (query group, reference group, strand), one after the other, then `sedef align bucket` on their files -- and `sedef
seeds`, one process.  Six records of 100 kb in three translation groups (SDF_TEST_TRANSLATE_LIMIT), every record but the first
with two 3 kb copies from the record before it, one of them inverted.  Every child process runs under a time limit of its own,
and the script stops at the first that fails.  Prints and writes the wall times, the index builds of both ways and whether the
bucket files agree.  A record of one run, not a gate: nobody fixed a ratio in advance.

    python profiles/seeds_cmd.py [--out FILE] [--records 6] [--bases 100000] [--bins 16]"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COMP = bytes.maketrans(b"ACGT", b"TGCA")


def genome(path, n_rec, n_bases, seed=3):
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGT", np.uint8)
    recs = [letters[rng.integers(0, 4, n_bases)].copy() for _ in range(n_rec)]
    for i in range(1, n_rec):
        for inverted in (False, True):
            src, dst = int(rng.integers(0, n_bases - 3000)), int(rng.integers(0, n_bases - 3000))
            piece = recs[i - 1][src:src + 3000].copy()
            flip = rng.random(3000) < 0.05
            piece[flip] = letters[rng.integers(0, 4, int(flip.sum()))]
            if inverted:
                piece = np.frombuffer(piece.tobytes().translate(COMP)[::-1], np.uint8)
            recs[i][dst:dst + 3000] = piece
    with open(path, "wb") as f, open(path + ".fai", "w") as fai:
        off = 0
        for i, r in enumerate(recs):
            head = b">r%d\n" % i
            body = b"\n".join(r[j:j + 60].tobytes() for j in range(0, n_bases, 60)) + b"\n"
            f.write(head + body)
            fai.write("r%d\t%d\t%d\t60\t61\n" % (i, n_bases, off + len(head)))
            off += len(head) + len(body)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seeds_cmd.txt"))
    ap.add_argument("--records", type=int, default=6)
    ap.add_argument("--bases", type=int, default=100000)
    ap.add_argument("--bins", type=int, default=16)
    ap.add_argument("--limit", type=int, default=120, help="seconds a child process may take")
    a = ap.parse_args()
    from sedef_amd import host
    host.build_host()
    lines = []

    def say(text):
        lines.append(text)
        print(text, flush=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    d = tempfile.mkdtemp(prefix="seeds_cmd_")
    fa = os.path.join(d, "genome.fa")
    genome(fa, a.records, a.bases)
    env = dict(os.environ, SDF_TEST_TRANSLATE_LIMIT=str(2 * a.bases))
    env.pop("SDF_BUCKET_DEVICE", None)

    def run(argv, stdout=subprocess.PIPE):
        t0 = time.perf_counter()
        p = subprocess.run([host.CLI] + argv, stdout=stdout, stderr=subprocess.PIPE, env=env, timeout=a.limit)
        if p.returncode != 0:
            say("FAILED (%d): %s\n%s" % (p.returncode, " ".join(argv), p.stderr.decode()[-1500:]))
            sys.exit(1)
        return time.perf_counter() - t0, p

    groups = int(run(["translate", fa])[1].stdout)
    say("sedef seeds against sedef.sh's seeding phase: %d records of %d bases in %d groups, %d bins; SDF_SEARCH_LANES=%s" % (
        a.records, a.bases, groups, a.bins, env.get("SDF_SEARCH_LANES", "unset")))
    old_seeds, old_buckets = os.path.join(d, "old_seeds"), os.path.join(d, "old_buckets")
    os.makedirs(old_seeds)
    os.makedirs(old_buckets)
    t_search, builds, procs, hits = 0.0, 0, 0, 0
    for j in range(groups):
        for i in range(j, groups):
            for m, flag in (("n", []), ("y", ["-r"])):
                with open(os.path.join(old_seeds, "%d_%d_%s.bed" % (i, j, m)), "wb") as f:
                    t, p = run(["search"] + flag + ["-t", fa, str(i), str(j)], stdout=f)
                t_search += t
                procs += 1
                builds += int(re.search(r"Indexes built: (\d+) for", p.stderr.decode()).group(1))
                hits += int(re.search(r"Total:\s+=\s+(\d+)", p.stderr.decode()).group(1))
    t_bucket, _ = run(["align", "bucket", "-n", str(a.bins), old_seeds, old_buckets, fa])
    say("old way: %d search processes %.2f s + align bucket %.2f s = %.2f s wall; %d indexes built, %d seed hits" % (
        procs, t_search, t_bucket, t_search + t_bucket, builds, hits))
    new_buckets = os.path.join(d, "new_buckets")
    t_new, p = run(["seeds", "-n", str(a.bins), fa, new_buckets])
    log = p.stderr.decode()
    same = all(open(os.path.join(old_buckets, n), "rb").read() == open(os.path.join(new_buckets, n), "rb").read() for n in sorted(os.listdir(old_buckets)))
    say("sedef seeds: %.2f s wall; %s indexes built, %s seed hits; bucket files %s; records path %s" % (
        t_new, re.search(r"Indexes built: (\d+) for", log).group(1), re.search(r"Total:\s+=\s+(\d+)", log).group(1),
        "byte-identical" if same and sorted(os.listdir(old_buckets)) == sorted(os.listdir(new_buckets)) else "DIFFER",
        "ignored (host path)" if "records path ignored" in log else "taken"))


if __name__ == "__main__":
    main()
