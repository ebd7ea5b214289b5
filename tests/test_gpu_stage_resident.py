"""`sedef align generate` on chromosomes that stay resident in HBM (SDF_STAGE_RESIDENT=1, sdfh_generate_many_resident): the
output is byte for byte what the super-batches that upload their own characters write."""
import os
import subprocess

import numpy as np
import pytest

from test_stage_pairs import _write_stage, golden, host  # noqa: F401  (fixtures and the fixture's materialiser)

pytestmark = pytest.mark.gpu

_COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "a": "t", "c": "g", "g": "c", "t": "a", "N": "N"}
CHROMS = (("chrA", 30000, 60), ("chrB", 24000, 50), ("chrC", 20011, 70))  # (name, bases, bases per line; chrC: a short last line)


def make_genome(d, seed, nsd=16, odd=False):
    """Three chromosomes with planted duplications inside and across them, on both strands, soft-masked stretches and an N
    run.  Returns (fasta path, {name: bases}, [(qname, a, rname, b, rc, length)])."""
    rng = np.random.default_rng(seed)
    alpha = np.array(list("ACGT"))
    seqs = {}
    for name, n, _ in CHROMS:
        s = alpha[rng.integers(0, 4, n)].astype("U1")
        for _ in range(n // 3000):
            a = int(rng.integers(0, n - 300))
            s[a:a + 250] = np.char.lower(s[a:a + 250])
        seqs[name] = s
    seqs["chrB"][5000:5040] = "N"
    dups = []
    for k in range(nsd):
        qn, qlen, _ = CHROMS[int(rng.integers(0, 3))]
        rn, rlen, _ = CHROMS[k % 3]
        L = 1500
        a = int(rng.integers(300, qlen // 2 - L - 300))
        b = int(rng.integers(rlen // 2 + 300, rlen - L - 600))
        out = []
        for c in seqs[qn][a:a + L]:
            x = rng.random()
            if x < 0.02:
                out.append(alpha[rng.integers(0, 4)])
            elif x < 0.025:
                continue
            elif x < 0.03:
                out += [c, alpha[rng.integers(0, 4)]]
            else:
                out.append(c)
        rc = bool(k % 2)
        if rc:
            out = [_COMP[c] for c in out[::-1]]
        out = out[:L]
        seqs[rn][b:b + len(out)] = out
        dups.append((qn, a, rn, b, rc, len(out)))
    if odd:  # characters that are no ACGTN inside the first duplication's query region
        qn, a = dups[0][0], dups[0][1]
        seqs[qn][a + 400] = "R"
        seqs[qn][a + 700] = "-"
    fa = os.path.join(str(d), "genome.fa")
    with open(fa, "w") as f, open(fa + ".fai", "w") as fai:
        at = 0
        for name, n, line in CHROMS:
            head = ">%s\n" % name
            f.write(head)
            at += len(head)
            fai.write("%s\t%d\t%d\t%d\t%d\n" % (name, n, at, line, line + 1))
            s = "".join(seqs[name])
            for i in range(0, n, line):
                f.write(s[i:i + line] + "\n")
                at += len(s[i:i + line]) + 1
    return fa, {name: n for name, n, _ in CHROMS}, dups


def write_buckets(d, dups, lens, n_buckets, pairs_per_bucket, seed, window=1000):
    rng = np.random.default_rng(seed)
    paths = []
    for b in range(n_buckets):
        p = os.path.join(str(d), "bucket_%04d" % b)
        with open(p, "w") as f:
            for _ in range(pairs_per_bucket):
                qn, a, rn, bb, rc, L = dups[int(rng.integers(0, len(dups)))]
                o = int(rng.integers(0, L - window))
                ro = L - window - o if rc else o  # (a reversed copy: the same bases lie at the other end)
                qs, rs = a + o + int(rng.integers(-40, 40)), bb + ro + int(rng.integers(-40, 40))
                f.write("%s\t%d\t%d\t%s\t%d\t%d\t\t\t+\t%s\t%d\t0\t\tOK\n" % (
                    qn, max(0, qs), min(lens[qn], qs + window), rn, max(0, rs), min(lens[rn], rs + window), "-" if rc else "+", window))
        paths.append(p)
    return paths


def outputs(buckets):
    return [open(b + ".aligned.bed", "rb").read() for b in buckets]


def test_fixture_stages_through_the_cli(host, golden, tmp_path):
    from sedef_amd.host import CLI
    for k, fx in enumerate(golden["stages"]):
        d = tmp_path / ("s%d" % k)
        d.mkdir()
        fa, bed = _write_stage(fx, d)
        want = "".join(line + "\n" for line in fx["expect"])
        got = {}
        for mode in ("1", "0"):
            env = dict(os.environ, SDF_STAGE_RESIDENT=mode, SDF_STAGE_WS_GIB="1")
            env.pop("SDF_DEVICES", None)
            r = subprocess.run([CLI, "align", "generate", "-k", str(fx["kmer"]), fa, bed], capture_output=True, text=True, env=env)
            assert r.returncode == 0, r.stderr[-2000:]
            got[mode] = r.stdout
            if mode == "1" and fx["kmer"] <= 15:
                assert "SDF_STAGE_RESIDENT=1 ignored" not in r.stderr, r.stderr[-2000:]
        assert got["1"] == want, k
        assert got["1"] == got["0"], k


def test_several_buckets_on_resident_chromosomes(host, tmp_path, monkeypatch):
    fa, lens, dups = make_genome(tmp_path, seed=31)
    assert any(d[4] for d in dups) and any(d[0] != d[2] for d in dups)
    buckets = write_buckets(tmp_path, dups, lens, 4, 128, seed=32)
    monkeypatch.delenv("SDF_DEVICES", raising=False)
    monkeypatch.delenv("SDF_STAGE_RESIDENT", raising=False)
    monkeypatch.setenv("SDF_STAGE_WS_GIB", "1")
    monkeypatch.setenv("SDF_SUPER_BATCH", "16")
    st0, tot0 = host.generate_many_resident(fa, buckets, 11, resident=False)
    want = outputs(buckets)
    assert sum(len(w) for w in want) > 0 and any(b"\t-\t" in w for w in want)
    assert tot0[3] == 0 and tot0[0] == 0 and tot0[2] == 4 * 8
    assert tot0[1] > sum(lens.values())
    for env in ({"SDF_LANES": "2", "SDF_SUPER_BATCH": "16"}, {"SDF_ANCHOR_PARTS": "3", "SDF_SUPER_BATCH": "64"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        for b in buckets:
            os.remove(b + ".aligned.bed")
        st, tot = host.generate_many_resident(fa, buckets, 11, resident=True)
        print(env, st, tot)
        assert outputs(buckets) == want, env
        assert st == st0
        assert tot[0] == len(lens) and tot[1] == sum(lens.values())
        assert tot[2] == 4 * (128 // int(env["SDF_SUPER_BATCH"])) and tot[3] == tot[2]
        assert tot[2] >= 2 * len(lens)
        for k in env:
            monkeypatch.delenv(k)


def test_a_pair_that_is_not_plain_acgtn(host, tmp_path, monkeypatch):
    """An `R` and a `-` inside a candidate region: the pair's match counters are recounted on the host in both modes."""
    fa, lens, dups = make_genome(tmp_path, seed=41, nsd=3, odd=True)
    qn, a, rn, b, rc, L = dups[0]
    bed = os.path.join(str(tmp_path), "bucket_0000")
    with open(bed, "w") as f:
        f.write("%s\t%d\t%d\t%s\t%d\t%d\t\t\t+\t%s\t%d\t0\t\tOK\n" % (qn, a - 100, a + L + 100, rn, b - 100, b + L + 100,
                                                                     "-" if rc else "+", L))
        qn2, a2, rn2, b2, rc2, L2 = dups[1]
        f.write("%s\t%d\t%d\t%s\t%d\t%d\t\t\t+\t%s\t%d\t0\t\tOK\n" % (qn2, a2 - 100, a2 + L2 + 100, rn2, b2 - 100, b2 + L2 + 100,
                                                                     "-" if rc2 else "+", L2))
    monkeypatch.delenv("SDF_DEVICES", raising=False)
    monkeypatch.delenv("SDF_STAGE_RESIDENT", raising=False)
    monkeypatch.setenv("SDF_STAGE_WS_GIB", "1")
    host.generate_many_resident(fa, [bed], 11, resident=False)
    want = outputs([bed])
    assert len(want[0]) > 0
    os.remove(bed + ".aligned.bed")
    _, tot = host.generate_many_resident(fa, [bed], 11, resident=True)
    assert tot[3] == tot[2] == 1
    assert outputs([bed]) == want
