"""Host pipeline above the C ABI (sedef_amd/csrc/host): Alignment / Hit / FASTA / chaining / refinement / driver.

CPU tests inject the CPU oracle as the DP through the library's test hook; GPU tests use the product path
(sdf_extz2_batch) and must reproduce the CPU-hook results byte for byte."""
import ctypes as C
import gzip
import json
import os
import re
import subprocess

import numpy as np
import pytest

import hostgen
from refcalls import ref_calls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host():
    from sedef_amd import host as h
    from sedef_amd.build import build_library
    build_library()
    h.build_host()
    return h


@pytest.fixture(scope="module")
def oracle_dp(oracle):
    return C.cast(oracle.lib.sdfo_extz2, C.c_void_p)


@pytest.fixture(scope="module")
def host_golden():
    with gzip.open(os.path.join(ROOT, "tests", "golden", "host_align_kat.json.gz"), "rb") as f:
        return json.loads(f.read().decode())


# ---------------------------------------------------------------- A1-A7, D2: pinned by the reference classes
def test_alignment_pair_matches_reference_golden(host, oracle_dp, host_golden):
    for c in host_golden["pairs"]:
        cig, cnt = host.alignment_pair(c["a"], c["b"], test_dp=oracle_dp)
        assert cig == c["cigar"] and cnt == c["counts"]


def test_chain_merge_guide_to_bed_match_reference_golden(host, oracle_dp, host_golden):
    assert len(host_golden["guides"]) >= 30
    for c in host_golden["guides"]:
        assert host.guide_from_chains(c["q"], c["r"], c["spec"], c["side"], test_dp=oracle_dp) == c["expect"]


def test_far_gap_of_equal_sides_keeps_its_zero_length_run(host, oracle_dp, host_golden):
    """qgap == rgap > 1000: the reference's far branch appends a run of length 0 (src/align.cc:135); invisible in a
    CIGAR string, but it counts as a gap and keeps the M runs on either side from merging ("...300M450M...")."""
    seen = 0
    for c in host_golden["far_equal"]:
        got = host.guide_from_chains(c["q"], c["r"], c["spec"], c["side"], test_dp=oracle_dp)
        assert got == c["expect"]
        import re as _re
        seen += bool(_re.search(r"\d+M\d+M", got))
    assert seen >= 2


def test_alignment_live_vs_reference_classes(host, oracle_dp):
    """(the reference's classes: live where oracle/_ref is built, else their recorded answers, tests/refcalls.py)"""
    from oracle.binding import ReferenceAlign
    with ref_calls("host_pipeline_alignment", ReferenceAlign) as ref:
        rng = np.random.default_rng(2)
        for it in range(120):
            a = hostgen.rseq(rng, int(rng.integers(1, 600)), 0.01 if it % 3 == 0 else 0)
            b = hostgen.mut(rng, a, rng.random() * 0.2)
            assert host.alignment_pair(a, b, test_dp=oracle_dp) == ref.alignment_pair(a, b)
        n = 0
        while n < 60:
            c = hostgen.chain_case(rng, host)
            if c is None:
                continue
            n += 1
            assert host.guide_from_chains(*c, test_dp=oracle_dp) == ref.guide_from_chains(*c)


def test_merge_matches_reference_golden(host, host_golden):
    assert len(host_golden["merges"]) >= 40
    for c in host_golden["merges"]:
        assert host.merge(c["lines"], 250) == c["expect"]


def test_merge_live_vs_reference(host):
    """(the reference's merge: live where oracle/_ref is built, else its recorded answers, tests/refcalls.py)"""
    from oracle.binding import ReferenceAlign
    with ref_calls("host_pipeline_merge", ReferenceAlign) as ref:
        rng = np.random.default_rng(8)
        for _ in range(200):
            lines, spec = hostgen.merge_case(rng)
            assert host.merge(lines, 250) == ref.merge(spec, 250)


def test_bucket_stage(host, oracle_dp, tmp_path):
    """`align bucket`: every seed ends up (extended, possibly merged) in exactly one bucket; buckets feed `generate`."""
    fa = str(tmp_path / "genome.fa")
    genome, beds = hostgen.make_genome(fa, seed=4, glen=80000, nsd=8)
    seeds = tmp_path / "seeds"
    seeds.mkdir()
    rng = np.random.default_rng(0)
    with open(seeds / "a.bed", "w") as f:  # several overlapping seeds per planted duplication
        for (a, e, b, e2, rcf) in beds:
            for _ in range(3):
                o = int(rng.integers(0, 300))
                f.write("chrT\t%d\t%d\tchrT\t%d\t%d\t\t\t+\t%s\t%d\t0\t\tOK\n" % (
                    a + o, a + o + 800, b + o, b + o + 800, "-" if rcf else "+", 800))
    out = tmp_path / "buckets"
    out.mkdir()
    host.bucket(str(seeds), 3, str(out), fa)
    files = sorted(os.listdir(out))
    assert files == ["bucket_0000", "bucket_0001", "bucket_0002"]
    lines = [ln for fn in files for ln in open(out / fn).read().splitlines()]
    assert 1 <= len(lines) <= len(beds) * 3
    for ln in lines:
        f = ln.split("\t")
        assert len(f) >= 12 and int(f[1]) < int(f[2]) and int(f[4]) < int(f[5]) and f[8] == "+"
    # merged + extended seeds cover the planted duplications; the buckets align
    res = tmp_path / "aligned.bed"
    total = 0
    for fn in files:
        st = host.generate(fa, str(out / fn), 11, str(res), test_dp=oracle_dp)
        total += st[1]
    assert total >= 4


# ---------------------------------------------------------------- D3 FASTA
def test_fasta_random_access(host, tmp_path):
    s, _ = hostgen.make_genome(str(tmp_path / "g.fa"), seed=3, glen=5000, nsd=0)
    fa = str(tmp_path / "g.fa")
    rng = np.random.default_rng(0)
    for _ in range(200):
        a = int(rng.integers(-5, 5100))
        b = int(rng.integers(a, 5300))
        got, end = host.fasta_get(fa, "chrT", a, b)
        aa = max(a, 0)
        assert end == min(b, 5000)
        assert got == s[aa:min(b, 5000)]
    with pytest.raises(RuntimeError):
        host.fasta_get(fa, "nope", 0, 10)


# ---------------------------------------------------------------- C1-C3: chaining invariants (parity unpinned)
def test_chains_are_exact_colinear_matches(host):
    rng = np.random.default_rng(9)
    for _ in range(20):
        q = hostgen.rseq(rng, 3000, 0.003)
        r = hostgen.rseq(rng, 200) + hostgen.mut(rng, q, 0.08) + hostgen.rseq(rng, 300)
        for chain in host.chains(q, r, 11):
            pq = pr = -1
            for (aq, ar, al, hu) in chain:
                assert al >= 11 and hu in (0, 1)
                assert q[aq:aq + al].upper() == r[ar:ar + al].upper() and "N" not in q[aq:aq + al].upper()
                # maximal to the right; strictly after the previous anchor in both sequences, gap <= 210
                assert aq + al == len(q) or ar + al == len(r) or q[aq + al].upper() != r[ar + al].upper() or \
                    "N" in (q[aq + al].upper(), r[ar + al].upper())
                if pq >= 0:
                    assert aq >= pq and ar >= pr and aq - pq <= 210 and ar - pr <= 210
                pq, pr = aq + al, ar + al


# ---------------------------------------------------------------- D1 + R1: the stage
def _check_bedpe(lines, genome):
    comp = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}
    for ln in lines:
        f = ln.split("\t")
        assert len(f) == 28
        qs, qe, rs, re_ = int(f[1]), int(f[2]), int(f[4]), int(f[5])
        ops = re.findall(r"(\d+)([MID])", f[12])
        qn = sum(int(n) for n, o in ops if o in "MD")
        rn = sum(int(n) for n, o in ops if o in "MI")
        assert qn == qe - qs and rn == re_ - rs and int(f[11]) == sum(int(n) for n, o in ops)
        assert int(f[11]) >= 900
        a = genome[qs:qe].upper()
        b = genome[rs:re_].upper()
        if f[9] == "-":
            b = "".join(comp[c] for c in b[::-1])
        i = j = mm = ma = 0
        for n, o in ops:
            n = int(n)
            if o == "M":
                for k in range(n):
                    if a[i + k] == b[j + k] and a[i + k] != "N":
                        ma += 1
                    else:
                        mm += 1
                i += n
                j += n
            elif o == "D":
                i += n
            else:
                j += n
        gb = sum(int(n) for n, o in ops if o != "M")
        assert f[13].startswith("m=%.1f;g=%.1f" % (100.0 * mm / (ma + mm + gb), 100.0 * gb / (ma + mm + gb)))


def test_generate_stage_cpu_hook(host, oracle_dp, tmp_path):
    fa = str(tmp_path / "genome.fa")
    genome, beds = hostgen.make_genome(fa, seed=1)
    out = str(tmp_path / "out.bed")
    lines, hits, tasks, cells, rounds = host.generate(fa, fa + ".bed", 11, out, test_dp=oracle_dp)
    assert lines == len(beds) and hits >= 4 and tasks > 50 and 2 <= rounds <= 6
    got = open(out).read().splitlines()
    assert len(got) == hits
    _check_bedpe(got, genome)
    # deterministic
    out2 = str(tmp_path / "out2.bed")
    host.generate(fa, fa + ".bed", 11, out2, test_dp=oracle_dp)
    assert open(out2).read() == open(out).read()


def test_cli_contract_without_gpu(host, tmp_path):
    """argv grammar / exit codes of the reference CLI (src/main.cc:104-157, src/align_main.cc:341-373)."""
    from sedef_amd.host import CLI
    r = subprocess.run([CLI], capture_output=True, text=True)
    assert r.returncode == 1 and "Arguments missing" in r.stderr
    r = subprocess.run([CLI, "align", "generate", "x.fa"], capture_output=True, text=True)
    assert r.returncode == 1 and "Error: Not enough arguments to align" in r.stderr and r.stdout == ""
    r = subprocess.run([CLI, "align", "generate", "x.fa", "y.bed"], capture_output=True, text=True)
    assert r.returncode == 1 and "Must provide k-mer size" in r.stderr
    r = subprocess.run([CLI, "help"], capture_output=True, text=True)
    assert r.returncode == 0
    import sedef_amd
    if sedef_amd.load_library().sdf_device_count() == 0:  # no HIP device: loud failure, no CPU fallback
        fa = str(tmp_path / "g.fa")
        hostgen.make_genome(fa, seed=2, glen=20000, nsd=1)
        r = subprocess.run([CLI, "align", "generate", "-k", "11", fa, fa + ".bed"], capture_output=True, text=True)
        assert r.returncode == 1 and "GPU DP backend unavailable" in r.stderr and r.stdout == ""


# ---------------------------------------------------------------- GPU: product path == CPU-hook path
@pytest.mark.gpu
def test_generate_stage_gpu_equals_cpu_hook(host, oracle_dp, tmp_path):
    from sedef_amd.host import CLI
    for seed, glen, nsd in ((1, 60000, 6), (5, 120000, 12)):
        fa = str(tmp_path / ("genome%d.fa" % seed))
        genome, beds = hostgen.make_genome(fa, seed=seed, glen=glen, nsd=nsd)
        cpu, gpu = str(tmp_path / "cpu.bed"), str(tmp_path / "gpu.bed")
        host.generate(fa, fa + ".bed", 11, cpu, test_dp=oracle_dp)
        host.generate(fa, fa + ".bed", 11, gpu)  # GPU provider
        assert open(gpu).read() == open(cpu).read()
        r = subprocess.run([CLI, "align", "generate", "-k", "11", fa, fa + ".bed"], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout == open(cpu).read() and "Finished" in r.stderr
        _check_bedpe(r.stdout.splitlines(), genome)


def test_generate_stage_lanes_keep_schedule_order_cpu_hook(host, oracle_dp, tmp_path, monkeypatch, capfd):
    """The driver's lane loop on the CPU hook (its providers clone like the device's): one, two and three lanes of
    super-batches write the same bytes in the same order."""
    fa = str(tmp_path / "genome.fa")
    hostgen.make_genome(fa, seed=9, glen=150000, nsd=14)
    monkeypatch.setenv("SDF_SUPER_BATCH", "2")  # 14 pairs -> 7 super-batches
    got = []
    for lanes in ("1", "2", "3"):
        monkeypatch.setenv("SDF_LANES", lanes)
        path = str(tmp_path / ("lanes%s.bed" % lanes))
        stats = host.generate(fa, fa + ".bed", 11, path, test_dp=oracle_dp)
        assert "%s lane(s)" % lanes in capfd.readouterr().err
        got.append(open(path, "rb").read())
        assert stats[0] == 14 and got[-1].count(b"\n") == stats[1] > 0
    assert got[1] == got[0] and got[2] == got[0]


@pytest.mark.gpu
def test_generate_stage_two_lanes_keep_schedule_order(host, oracle_dp, tmp_path, monkeypatch):
    """Super-batches on two device contexts at once (SDF_LANES): same bytes, same line order as one lane."""
    fa = str(tmp_path / "genome.fa")
    hostgen.make_genome(fa, seed=9, glen=150000, nsd=14)
    cpu, one, two = (str(tmp_path / n) for n in ("cpu.bed", "one.bed", "two.bed"))
    host.generate(fa, fa + ".bed", 11, cpu, test_dp=oracle_dp)
    monkeypatch.setenv("SDF_LANES", "1")
    host.generate(fa, fa + ".bed", 11, one)
    monkeypatch.setenv("SDF_LANES", "2")
    monkeypatch.setenv("SDF_SUPER_BATCH", "3")  # 14 pairs -> 5 super-batches over 2 lanes
    stats = host.generate(fa, fa + ".bed", 11, two)
    assert open(two).read() == open(one).read() == open(cpu).read()
    assert stats[0] == 14 and open(two).read().count("\n") == stats[1]
    monkeypatch.setenv("SDF_DEVICES", "0,0,0")  # lanes spread over a device list (here the same GPU three times)
    monkeypatch.delenv("SDF_LANES")
    three = str(tmp_path / "three.bed")
    host.generate(fa, fa + ".bed", 11, three)
    assert open(three).read() == open(cpu).read()
    # the product CLI sets its lanes up before the stage starts (spare providers made side by side with the first, buffers
    # sized from the BED file: host/sedef_main.cc, stage_hint) and takes the largest super-batches first
    from sedef_amd.host import CLI
    env = dict(os.environ, SDF_LANES="3", SDF_SUPER_BATCH="2")
    env.pop("SDF_DEVICES", None)
    r = subprocess.run([CLI, "align", "generate", "-k", "11", fa, fa + ".bed"], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and r.stdout == open(cpu).read() and "3 lane(s)" in r.stderr


def _buckets(host, tmp_path, seed=9, nsd=10, nb=3):
    fa = str(tmp_path / "genome.fa")
    genome, beds = hostgen.make_genome(fa, seed=seed, glen=90000, nsd=nsd)
    seeds = tmp_path / "seeds"
    seeds.mkdir()
    rng = np.random.default_rng(seed)
    with open(seeds / "a.bed", "w") as f:
        for (a, e, b, e2, rcf) in beds:
            o = int(rng.integers(0, 200))
            f.write("chrT\t%d\t%d\tchrT\t%d\t%d\t\t\t+\t%s\t%d\t0\t\tOK\n" % (
                a + o, a + o + 900, b + o, b + o + 900, "-" if rcf else "+", 900))
    out = tmp_path / "align"
    out.mkdir()
    host.bucket(str(seeds), nb, str(out), fa)
    return fa, out, sorted(str(out / n) for n in os.listdir(out))


def test_several_buckets_in_one_run_equal_one_bucket_runs(host, oracle_dp, tmp_path):
    """generate_many: one provider, bucket after bucket -- every bucket's file is what its own run writes; the directory
    form takes `bucket_????` files only (not the outputs next to them)."""
    fa, out, buckets = _buckets(host, tmp_path)
    assert len(buckets) == 3
    want = []
    for b in buckets:
        host.generate(fa, b, 11, b + ".single", test_dp=oracle_dp)
        want.append(open(b + ".single").read())
    assert sum(len(w) for w in want) > 0
    logs = tmp_path / "logs"
    logs.mkdir()
    st = host.generate_many(fa, buckets, 11, log_dir=str(logs), test_dp=oracle_dp)
    assert [open(b + ".aligned.bed").read() for b in buckets] == want
    assert [x[0] for x in st] == [sum(1 for _ in open(b)) for b in buckets]
    assert sorted(os.listdir(logs)) == [os.path.basename(b) + ".log" for b in buckets]
    assert all("Finished BED" in open(logs / n).read() for n in os.listdir(logs))
    for b in buckets:
        os.remove(b + ".aligned.bed")
    st2 = host.generate_many(fa, [str(out)], 11, test_dp=oracle_dp)  # the directory: the three bucket files, in order
    assert st2 == st and [open(b + ".aligned.bed").read() for b in buckets] == want


@pytest.mark.parametrize("lanes", ["1", "2"])
def test_several_buckets_one_missing_fails_with_its_name(host, oracle_dp, tmp_path, monkeypatch, lanes):
    """A bucket file that cannot be read ends the run with an error that names it (the CLI: exit code 1), whether the
    buckets run one after the other or two at a time; the buckets done before it keep their complete outputs."""
    fa, out, buckets = _buckets(host, tmp_path, seed=23, nsd=8, nb=3)
    monkeypatch.setenv("SDF_BUCKET_LANES", lanes)
    missing = str(out / "bucket_9999")
    with pytest.raises(Exception) as e:
        host.generate_many(fa, buckets[:1] + [missing] + buckets[1:], 11, test_dp=oracle_dp)
    assert "bucket_9999" in str(e.value)
    host.generate(fa, buckets[0], 11, buckets[0] + ".single", test_dp=oracle_dp)
    assert open(buckets[0] + ".aligned.bed").read() == open(buckets[0] + ".single").read()


@pytest.mark.parametrize("lanes", ["1", "2", "3"])
def test_buckets_in_flight_write_what_one_after_the_other_writes(host, oracle_dp, tmp_path, monkeypatch, lanes):
    """SDF_BUCKET_LANES buckets of a several-bucket run are in flight at a time, each on a provider of its own (default 2):
    every bucket's file and the per-bucket figures are those of buckets done one after the other; without --log-dir each
    bucket's log lines reach the shared log in one piece."""
    fa, out, buckets = _buckets(host, tmp_path, seed=21, nsd=16, nb=5)
    want = []
    for b in buckets:
        host.generate(fa, b, 11, b + ".single", test_dp=oracle_dp)
        want.append(open(b + ".single").read())
    assert sum(len(w) for w in want) > 0
    monkeypatch.setenv("SDF_BUCKET_LANES", lanes)
    st = host.generate_many(fa, buckets, 11, test_dp=oracle_dp)
    assert [open(b + ".aligned.bed").read() for b in buckets] == want
    assert [x[0] for x in st] == [sum(1 for _ in open(b)) for b in buckets]
    assert [x[1] for x in st] == [w.count("\n") for w in want]


@pytest.mark.gpu
def test_cli_several_buckets_one_process_gpu(host, tmp_path):
    """`sedef align generate -k 11 genome.fa bucket_0000 bucket_0001 ...` and `... genome.fa align/`: one process, lanes and
    device contexts set up once; every b.aligned.bed byte-identical to `sedef align generate ... b > b.aligned.bed`."""
    from sedef_amd.host import CLI
    fa, out, buckets = _buckets(host, tmp_path, seed=12, nsd=14, nb=4)
    env = dict(os.environ)
    env.pop("SDF_DEVICES", None)
    want = []
    for b in buckets:
        r = subprocess.run([CLI, "align", "generate", "-k", "11", fa, b], capture_output=True, text=True, env=env)
        assert r.returncode == 0 and "Finished BED" in r.stderr
        want.append(r.stdout)
    assert sum(len(w) for w in want) > 0
    logs = tmp_path / "logs"
    logs.mkdir()
    for args, e in ((buckets, env), ([str(out)], dict(env, SDF_LANES="3", SDF_SUPER_BATCH="2")),
                    (buckets, dict(env, SDF_BUCKET_LANES="1")), ([str(out)], dict(env, SDF_BUCKET_LANES="3"))):
        for b in buckets:
            if os.path.exists(b + ".aligned.bed"):
                os.remove(b + ".aligned.bed")
        r = subprocess.run([CLI, "align", "generate", "-k", "11", "--log-dir", str(logs), fa] + args, capture_output=True,
                           text=True, env=e)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stdout == ""
        assert [open(b + ".aligned.bed").read() for b in buckets] == want
        assert r.stderr.count("Finished BED") == len(buckets) and "All 4 buckets done" in r.stderr
        assert sum("Finished" in open(logs / n).read() for n in os.listdir(logs)) == len(buckets)  # (sedef.sh:195)


@pytest.mark.gpu
def test_alignment_golden_on_gpu(host, host_golden):
    for c in host_golden["pairs"]:
        cig, cnt = host.alignment_pair(c["a"], c["b"])
        assert cig == c["cigar"] and cnt == c["counts"]
    for c in host_golden["guides"]:
        assert host.guide_from_chains(c["q"], c["r"], c["spec"], c["side"]) == c["expect"]
    # Alignment::merge runs inside the guides above (overlapping neighbours, src/refine.cc:172); the far gap of equal sides
    # with its zero-length run (src/align.cc:135), the CLI's scoring overrides and the hit-level merge() of src/merge.cc
    # (no DP in it: the same host code whichever provider is loaded) complete the reference-generated sections
    for c in host_golden["far_equal"]:
        assert host.guide_from_chains(c["q"], c["r"], c["spec"], c["side"]) == c["expect"]
    for c in host_golden["scored"]:
        cig, cnt = host.alignment_pair(c["a"], c["b"], scoring=c["scoring"])
        assert cig == c["cigar"] and cnt == c["counts"]
    for c in host_golden["merges"]:
        assert host.merge(c["lines"], 250) == c["expect"]


@pytest.mark.gpu
def test_gpu_anchors_equal_host_anchors(host):
    """sdf_anchors_batch (GPU sort/search/scan) returns exactly generate_anchors' list, in its order."""
    import sedef_amd
    eng = sedef_amd.Extz2Engine(0)
    rng = np.random.default_rng(17)
    pairs = []
    for it in range(40):
        q = hostgen.rseq(rng, int(rng.integers(5, 4000)), 0.004 if it % 2 else 0.0)
        r = hostgen.rseq(rng, int(rng.integers(0, 300))) + hostgen.mut(rng, q, rng.random() * 0.1) + \
            hostgen.rseq(rng, int(rng.integers(0, 300)))
        if it % 5 == 0:  # low-complexity stretch below the cap: at most 258 occurrences of a k-mer (the cap: test_gpu_anchor_edges.py)
            rep = "ACGTTGCAACGT" * 200
            q, r = q[:500] + rep + q[500:], r[:300] + rep + rep[:700] + r[300:]
        same = it % 3 == 0
        pairs.append((q, r, same, int(rng.integers(-30, 30)) if same else 0))
    pairs.append(("ACGT", "ACGTACGTACGTACGT", False, 0))  # shorter than k
    got = eng.anchors_batch(pairs, 11)
    for (q, r, same, delta), g in zip(pairs, got):
        exp = host.anchors(q, r, 11, same_chr=same, qstart=0, rstart=delta)
        assert g == exp, (len(q), len(r), same, delta, len(g), len(exp))


def _chain_cases(host):
    rng = np.random.default_rng(23)
    cases = [np.zeros((0, 4), np.int32), np.array([[5, 9, 11, 1]], np.int32),
             np.array([[0, 0, 12, 0], [30, 31, 15, 1]], np.int32),
             np.array([[0, 0, 12, 0], [30, 31, 15, 1], [400, 80, 11, 0]], np.int32)]
    for it in range(30):  # anchors of mutated copies: real chains, gaps, repeats
        q = hostgen.rseq(rng, int(rng.integers(50, 6000)), 0.004 if it % 2 else 0.0)
        r = hostgen.rseq(rng, int(rng.integers(0, 300))) + hostgen.mut(rng, q, rng.random() * 0.15) + \
            hostgen.rseq(rng, int(rng.integers(0, 300)))
        if it % 4 == 0:
            rep = "ACGTTGCAACGT" * 40
            q, r = q[:200] + rep + q[200:], r[:100] + rep + r[100:]
        cases.append(np.array(host.anchors(q, r, 11), np.int32).reshape(-1, 4))
    for it in range(30):  # random anchor sets with many equal scores and coordinates (tie order)
        m = int(rng.integers(1, 400))
        span = int(rng.integers(20, 3000))
        a = np.stack([rng.integers(0, span, m), rng.integers(0, span, m), rng.integers(11, 14, m),
                      rng.integers(0, 2, m)], 1).astype(np.int32)
        cases.append(a)
    return cases


@pytest.mark.gpu
def test_gpu_chains_equal_host_chains(host):
    """sdf_chain_batch (one wavefront per pair, everything in LDS, at these sizes; tests/test_gpu_chain_paths.py runs the
    thread-per-pair kernel) returns chain_anchors' path and boundaries exactly."""
    import sedef_amd
    eng = sedef_amd.Extz2Engine(0)
    cases = _chain_cases(host)
    for gap, score in ((210, 4), (50, 3), (1000, 5)):
        got = eng.chain_batch(cases, gap, score)
        for a, (gp, gb) in zip(cases, got):
            ep, eb = host.chain_raw(a, gap, score)
            assert np.array_equal(gp, ep) and np.array_equal(gb, eb), (len(a), gap, score)
    assert eng.chain_batch([]) == []
