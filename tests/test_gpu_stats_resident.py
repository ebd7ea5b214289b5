"""GPU: the stats columns of alignments that name ranges of the RESIDENT pool, with a strand per side
(sdf_stats_columns_pairs / sdf_stats_columns_pairs_device, SDF_STATS_A_RC / SDF_STATS_B_RC; stats_cols.hip: the <true> kernels),
and `stats generate` on resident chromosomes (StatsParams::resident).

No expected value comes from the code under test: either the CPU oracle (oracle/stats_oracle.c) on strings that were
reverse-complemented on the host -- the 128-entry table through sedef_amd.host.sequence, which restates the reference's
rev_dna -- or sdf_stats_columns_batch, the call as it was, on a pool into which the reversed ranges were written forward."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch  # (at collection: before the library brings a HIP runtime of its own along)

from oracle.binding import STATS_FIELDS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu

UNSUPPORTED, INVALID = -3, -4  # SDF_ERR_UNSUPPORTED, SDF_ERR_INVALID
EDGE = (0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65)  # around the eight-byte unit and the 64 lanes


def rev_table():
    """kDna.rev (sedef_amd/csrc/host/alignment.cc; reference: src/common.h:72-77) through the host library's Sequence ctor."""
    from sedef_amd import host
    host.build_host()
    chars = "".join(chr(c) for c in range(1, 128))
    _, rc, _ = host.sequence("t", chars, True)
    assert len(rc) == 127
    tab = np.full(128, ord("N"), np.uint8)
    tab[1:] = np.frombuffer(rc.encode("latin-1"), np.uint8)[::-1]
    tab = np.concatenate([tab, tab])  # (the table is indexed with c & 127)
    assert bytes(tab[[65, 67, 71, 84, 97, 99, 103, 116, 78, 110, 82]]) == b"TGCAtgcaNNN"
    return tab


@pytest.fixture(scope="module")
def tab():
    return rev_table()


def make_pool(rng, n):
    """Mixed case in short stretches, N and n runs, IUPAC letters and '-': every kind of byte within any eight."""
    a = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].copy()
    pos = 0
    while pos < n:
        L = int(rng.integers(2, 40))
        if rng.random() < 0.4:
            a[pos:pos + L] |= 0x20
        pos += L
    for _ in range(max(2, n // 250)):
        s = int(rng.integers(0, n))
        a[s:s + int(rng.integers(1, 13))] = ord("N") if rng.random() < 0.6 else ord("n")
    k = max(4, n // 30)
    a[rng.integers(0, n, k)] = np.frombuffer(b"RYKMSWrykmX-*-", np.uint8)[rng.integers(0, 14, k)]
    return a


def words(runs):
    return np.array([(l << 4) | op for op, l in runs], np.uint32)


def fit(want, a_len, b_len):
    """The runs of `want`, cut where the sequences run out (op 0 'M', 1 'D': a only, 2 'I': b only)."""
    runs, ia, ib = [], 0, 0
    for op, l in want:
        room = min(a_len - ia if op != 2 else l, b_len - ib if op != 1 else l)
        l = min(l, room)
        if l <= 0:
            continue
        runs.append((op, l))
        ia += l if op != 2 else 0
        ib += l if op != 1 else 0
    return runs


def build(specs):
    """specs: (a_off, a_len, b_off, b_len, runs, a_rc, b_rc) -> tasks, CIGAR words, a_rc, b_rc."""
    from sedef_amd.extz2 import STATS_TASK_DTYPE
    tasks = np.zeros(len(specs), STATS_TASK_DTYPE)
    cig, at = [], 0
    for k, (ao, al, bo, bl, runs, _, _) in enumerate(specs):
        tasks[k] = (ao, bo, al, bl, at, len(runs), 0)
        cig.append(words(runs))
        at += len(runs)
    cig = np.concatenate(cig) if cig else np.zeros(0, np.uint32)
    return tasks, cig, np.array([s[5] for s in specs], bool), np.array([s[6] for s in specs], bool)


def sides(tab, pool, spec):
    ao, al, bo, bl, runs, a_rc, b_rc = spec
    a, b = pool[ao:ao + al], pool[bo:bo + bl]
    return (tab[a[::-1]] if a_rc else a).tobytes(), (tab[b[::-1]] if b_rc else b).tobytes()


def oracle_cols(oracle, tab, pool, specs):
    """The oracle on strings reverse-complemented on the host: one row of sixteen counters per alignment."""
    out = np.zeros((len(specs), 16), np.int64)
    for k, s in enumerate(specs):
        a, b = sides(tab, pool, s)
        out[k] = oracle.stats_columns(a, b, words(s[4]))
    return out


def as_rows(cols):
    return np.stack([cols[f].astype(np.int64) for f in STATS_FIELDS], axis=1)


def check(eng, oracle, tab, pool, specs, exp=None):
    tasks, cig, a_rc, b_rc = build(specs)
    got = as_rows(eng.stats_columns_pairs(tasks, cig, a_rc=a_rc, b_rc=b_rc))
    exp = oracle_cols(oracle, tab, pool, specs) if exp is None else exp
    bad = np.flatnonzero((got != exp).any(axis=1))
    assert len(bad) == 0, (len(bad), specs[bad[0]][:4], specs[bad[0]][5:], got[bad[0]].tolist(), exp[bad[0]].tolist())
    return exp


def random_specs(rng, pool_len, n, max_runs, strands=None, min_runs=1, max_len=39):
    """n alignments of min_runs .. max_runs runs somewhere in the pool; every fourth CIGAR stops short of its sequences."""
    specs = []
    for k in range(n):
        nr = int(rng.integers(min_runs, max_runs + 1))
        runs = [(int(rng.choice([0, 0, 0, 1, 2])), int(rng.integers(0 if k % 5 == 0 else 1, max_len + 1))) for _ in range(nr)]
        na, nb = sum(l for op, l in runs if op != 2), sum(l for op, l in runs if op != 1)
        al, bl = na + (3 if k % 4 == 0 else 0), nb + (k % 4 == 0)
        s = int(rng.integers(0, 4)) if strands is None else strands
        specs.append((int(rng.integers(0, pool_len - al + 1)), al, int(rng.integers(0, pool_len - bl + 1)), bl, runs,
                      bool(s & 1), bool(s & 2)))
    return specs


def _pool_read(eng, off, n):
    buf = np.zeros(max(n, 1), np.uint8)
    eng.lib.sdf_debug_pool_read.restype = C.c_int
    eng.lib.sdf_debug_pool_read.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]
    assert eng.lib.sdf_debug_pool_read(eng.ctx, off, n, buf.ctypes.data) == 0
    return buf[:n]


# ---- 1. the edges of the eight-byte fetch ----------------------------------------------------------------------------------------
def test_fetch_edges_at_both_ends_of_the_pool_and_inside(oracle, tab):
    import sedef_amd
    rng = np.random.default_rng(11)
    pool = make_pool(rng, 4099)
    P = len(pool)
    cigars = ("single M", [(0, 3), (1, 2), (0, 9), (2, 4), (0, 7)], [(0, 8), (1, 1), (0, 16), (2, 1), (0, 8), (1, 8), (0, 16)])
    specs = []
    for place in range(3):
        for al in EDGE:
            for bl in EDGE:
                for strand in range(4):
                    for ci, want in enumerate(cigars):
                        if ci == 1:  # M D M I M with runs of 1..9
                            want = [(op, int(rng.integers(1, 10))) for op, _ in want]
                        runs = [(0, min(al, bl))] if ci == 0 else fit(want, al, bl)
                        ao, bo = ((0, 0), (P - al, P - bl), (1001 + 3 * strand, 2003 + 5 * ci))[place]
                        specs.append((ao, al, bo, bl, runs, bool(strand & 1), bool(strand & 2)))
    assert any(s[0] == 0 and s[5] for s in specs) and any(s[0] + s[1] == P and s[5] and s[1] == 65 for s in specs)
    eng = sedef_amd.Extz2Engine(0)
    assert eng.pool_upload(pool.tobytes()) == P
    exp = check(eng, oracle, tab, pool, specs)
    assert (exp[:, 15] == 0).all() and (exp[:, 3] > 0).sum() > len(specs) // 2
    # the strands matter: without the bits the same tasks count differently
    tasks, cig, _, _ = build(specs)
    plain = as_rows(eng.stats_columns_pairs(tasks, cig))
    assert (plain != exp).any(axis=1).sum() > len(specs) // 4
    eng.close()


def test_bytes_outside_ascii_next_to_a_reversed_side(oracle, tab):
    """A forward side with bytes >= 0x80 sends its unit down the per-column path while the other side of the same unit was
    reversed and complemented; a reversed side with such bytes reads them as rev_dna(c & 127)."""
    import sedef_amd
    a = np.frombuffer(b"AC\xc3\x80GTacgtNNAC\xffTACGTACGTAC\xc1\xe7tgcaACGTTGCA", np.uint8)
    b = np.frombuffer(b"TGCAACGTtgcaGTACGTACGTAGTNnacgtACTTGCAGT", np.uint8)
    pool = np.concatenate([a, b, np.arange(1, 256, dtype=np.uint8)])
    hi = len(a) + len(b)
    specs = []
    for strand in range(4):
        specs.append((0, len(a), len(a), len(b), [(0, 12), (1, 2), (0, 12), (2, 3), (0, 10)], bool(strand & 1), bool(strand & 2)))
        specs.append((hi, 255, 0, len(a), [(0, 9), (1, 200), (0, 30)], bool(strand & 1), bool(strand & 2)))
        specs.append((hi, 255, hi, 255, [(0, 255)], bool(strand & 1), bool(strand & 2)))
    eng = sedef_amd.Extz2Engine(0)
    eng.pool_upload(pool.tobytes())
    check(eng, oracle, tab, pool, specs)
    eng.close()


# ---- 2. four short alignments in one wavefront -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_pool():
    return make_pool(np.random.default_rng(12), 20011)


def test_groups_with_a_strand_per_row(oracle, tab, big_pool):
    import sedef_amd
    rng = np.random.default_rng(13)
    specs = random_specs(rng, len(big_pool), 64, 16)
    quads = [tuple((s[5], s[6]) for s in specs[q:q + 4]) for q in range(0, 64, 4)]
    assert sum(len(set(q)) > 1 for q in quads) >= 12  # the rows of a wavefront differ
    exp = oracle_cols(oracle, tab, big_pool, specs)
    for settings in ({}, dict(SDF_STATS_GROUP_MAX=0), dict(SDF_STATS_GROUP_MAX=64)):
        eng = sedef_amd.Extz2Engine(0, config=settings)
        eng.pool_upload(big_pool.tobytes())
        check(eng, oracle, tab, big_pool, specs, exp)
        eng.close()


# ---- 3. the segments of a long alignment --------------------------------------------------------------------------------------------
def test_segments_of_a_long_alignment_on_either_strand(oracle, tab, big_pool):
    import sedef_amd
    rng = np.random.default_rng(14)
    runs = []
    for k in range(750):
        runs += [(0, int(rng.integers(1, 14))), (int(rng.integers(1, 3)), int(rng.integers(0 if k % 97 == 0 else 1, 4)))]
    assert len(runs) == 1500
    na, nb = sum(l for op, l in runs if op != 2), sum(l for op, l in runs if op != 1)
    assert 5000 < na < 7500 and 5000 < nb < 7500
    short = random_specs(rng, len(big_pool), 20, 30)
    calls = []
    for strand in range(4):
        # (the long one in the middle of the short ones; its ranges end at the pool's last byte / start at byte 0)
        long_ = (len(big_pool) - na - 2, na + 2, 0, nb, runs, bool(strand & 1), bool(strand & 2))
        calls.append(short[:7] + [long_] + short[7:])
    exps = [oracle_cols(oracle, tab, big_pool, specs) for specs in calls]
    for settings in ({}, dict(SDF_STATS_ITEMS=1)):  # (a list of one segment: the alignment is counted whole)
        eng = sedef_amd.Extz2Engine(0, config=settings)
        eng.pool_upload(big_pool.tobytes())
        for specs, exp in zip(calls, exps):
            check(eng, oracle, tab, big_pool, specs, exp)
        eng.close()
    assert len({e[7].tobytes() for e in exps}) == 4  # the four strand combinations count differently


# ---- 4. FASTA-layout upload ------------------------------------------------------------------------------------------------------------
def test_ranges_of_records_appended_as_the_file_has_them(tab):
    import sedef_amd
    from test_resident_strand_cpu import fasta_lines
    rng = np.random.default_rng(15)
    recs = [(make_pool(rng, 60 * 31 + 17), 60, True), (make_pool(rng, 7 * 290 + 3), 7, False)]  # (the last lines are short)
    eng = sedef_amd.Extz2Engine(0)
    base = []
    for i, (seq, width, last_eol) in enumerate(recs):
        raw = fasta_lines(seq.tobytes(), width, b"\n", last_eol)
        assert raw.endswith(b"\n") == last_eol
        base.append(eng.pool_append_fasta(raw, len(seq), width, width + 1, reset=(i == 0)))
    assert base == [0, len(recs[0][0])] and eng.pool_bytes() == sum(len(r[0]) for r in recs)
    specs, alns = [], []
    for k in range(200):
        ra, rb = int(rng.integers(0, 2)), int(rng.integers(0, 2))
        s = random_specs(rng, 1 << 20, 1, 40, strands=0)[0]  # (lengths and runs; the offsets are chosen below)
        runs, al, bl = s[4], s[1], s[3]
        ax, bx = int(rng.integers(0, len(recs[ra][0]) - al + 1)), int(rng.integers(0, len(recs[rb][0]) - bl + 1))
        strand = 0 if k % 2 == 0 else int(rng.integers(1, 4))
        specs.append((base[ra] + ax, al, base[rb] + bx, bl, runs, bool(strand & 1), bool(strand & 2)))
        a, b = recs[ra][0][ax:ax + al], recs[rb][0][bx:bx + bl]
        alns.append(((tab[a[::-1]] if strand & 1 else a).tobytes(), (tab[b[::-1]] if strand & 2 else b).tobytes(), words(runs)))
    assert sum(s[5] or s[6] for s in specs) == 100
    tasks, cig, a_rc, b_rc = build(specs)
    got = eng.stats_columns_pairs(tasks, cig, a_rc=a_rc, b_rc=b_rc)
    old = sedef_amd.Extz2Engine(0)
    exp = old.stats_columns_batch(alns)  # today's call on host-prepared bytes
    assert got.tobytes() == exp.tobytes() and int(exp["match_b"].sum()) > 1000
    eng.close()
    old.close()


# ---- 5. the contract ---------------------------------------------------------------------------------------------------------------------
def test_contract_of_the_host_form(oracle, tab):
    import sedef_amd
    from sedef_amd.extz2 import STATS_COLS_DTYPE, SdfError
    rng = np.random.default_rng(16)
    pool = make_pool(rng, 3001)
    P = len(pool)
    eng = sedef_amd.Extz2Engine(0)
    assert eng.pool_upload(pool.tobytes()) == P
    good = random_specs(rng, P, 12, 20)
    tasks, cig, a_rc, b_rc = build(good)

    def unchanged():
        assert eng.pool_bytes() == P and _pool_read(eng, 0, P).tobytes() == pool.tobytes()

    def refused(rc, t, **kw):
        with pytest.raises(SdfError, match="rc=%d" % rc) as e:
            eng.stats_columns_pairs(t, cig, **kw)
        unchanged()
        return str(e.value)

    t = tasks.copy()
    t["reserved"][5] = 0x4
    assert "unknown stats task flag" in refused(UNSUPPORTED, t)
    t["reserved"][5] = 0x80000001
    assert "unknown stats task flag" in refused(UNSUPPORTED, t)
    for side in "ab":  # one byte past the pool
        t = tasks.copy()
        t[side + "_off"][3] = P - int(t[side + "_len"][3]) + 1
        refused(INVALID, t, a_rc=a_rc, b_rc=b_rc)
    t = tasks.copy()
    t["cigar_off"][11] = len(cig) - int(t["n_cigar"][11]) + 1  # a CIGAR range one word past its pool
    refused(INVALID, t)
    t = tasks.copy()
    t["a_len"][0] = (1 << 24) + 1  # (checked before any launch: no such pool is needed)
    assert "16 Mb" in refused(UNSUPPORTED, t)
    # a CIGAR longer than a REVERSED side: flags == 1 on that record, every other record as the oracle has it
    specs = list(good)
    ao, al, bo, bl, runs, _, _ = specs[4]
    specs[4] = (ao, al, P - bl, bl, runs + [(2, 1), (0, 1)], False, True)
    specs[9] = specs[9][:5] + (True, True)
    t, c2, ar, br = build(specs)
    out = np.zeros(len(specs), STATS_COLS_DTYPE)
    with pytest.raises(SdfError, match="rc=%d: alignment 4: the CIGAR does not fit" % INVALID):
        eng.stats_columns_pairs(t, c2, a_rc=ar, b_rc=br, out=out)
    unchanged()
    exp = oracle_cols(oracle, tab, pool, specs)
    assert int(out["flags"][4]) == 1 and exp[4][15] == 1
    keep = np.arange(len(specs)) != 4
    assert (as_rows(out)[keep] == exp[keep]).all()
    # nothing to do
    assert len(eng.stats_columns_pairs(tasks[:0], cig)) == 0
    assert eng.lib.sdf_stats_columns_pairs(eng.ctx, None, 0, None, 0, None) == 0
    unchanged()
    # the context serves a correct call afterwards
    check(eng, oracle, tab, pool, good)
    unchanged()
    eng.close()
    # an empty pool holds no non-empty range (and every empty one)
    empty = sedef_amd.Extz2Engine(0)
    assert empty.pool_bytes() == 0
    with pytest.raises(SdfError, match="rc=%d" % INVALID):
        empty.stats_columns_pairs(tasks[:1], cig)
    assert empty.pool_bytes() == 0
    z = tasks[:2].copy()
    z["a_off"], z["b_off"], z["a_len"], z["b_len"], z["cigar_off"], z["n_cigar"] = 0, 0, 0, 0, 0, 0
    got = empty.stats_columns_pairs(z, cig, b_rc=True)
    assert not as_rows(got).any()
    empty.close()


# ---- 6. the existing calls never read `reserved` -----------------------------------------------------------------------------------------
def test_existing_batch_call_ignores_reserved(tab, big_pool):
    import sedef_amd
    from sedef_amd.extz2 import STATS_COLS_DTYPE
    rng = np.random.default_rng(17)
    specs = random_specs(rng, len(big_pool), 90, 40) + random_specs(rng, len(big_pool), 2, 1400, min_runs=1100, max_len=12)
    tasks, cig, _, _ = build(specs)
    eng = sedef_amd.Extz2Engine(0)
    outs = []
    for reserved in (0, 3):
        t = tasks.copy()
        t["reserved"] = reserved
        out = np.zeros(len(t), STATS_COLS_DTYPE)
        eng._check(eng.lib.sdf_stats_columns_batch(eng.ctx, t.ctypes.data, len(t), big_pool.tobytes(), len(big_pool), cig.ctypes.data,
                                                   len(cig), out.ctypes.data))
        outs.append(out)
    assert outs[0].tobytes() == outs[1].tobytes()
    assert (outs[0]["flags"] == 0).all() and int(outs[0]["aln_b"].sum()) > 10000 and int(tasks["n_cigar"].max()) > 1024
    eng.close()


# ---- 7. the device form --------------------------------------------------------------------------------------------------------------------
def test_device_form_equals_host_form(big_pool):
    import sedef_amd
    from sedef_amd.extz2 import STATS_A_RC, STATS_B_RC, STATS_COLS_DTYPE
    rng = np.random.default_rng(18)
    specs = random_specs(rng, len(big_pool), 150, 40) + random_specs(rng, len(big_pool), 1, 1300, min_runs=1100, max_len=12)
    tasks, cig, a_rc, b_rc = build(specs)
    eng = sedef_amd.Extz2Engine(0)
    eng.pool_upload(big_pool.tobytes())
    dev = torch.device("cuda", 0)

    def on_device(t, any_rc, stream):
        d_tasks = torch.from_numpy(t.view(np.uint8).copy()).to(dev)
        d_cig = torch.from_numpy(cig.view(np.int32).copy()).to(dev)
        d_out = torch.full((len(t) * 16,), -1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        eng.pool_sync()  # (the pool's upload ran on the context's stream)
        eng.stats_columns_pairs_device(d_tasks.data_ptr(), len(t), any_rc, d_cig.data_ptr(), d_out.data_ptr(),
                                       stream.cuda_stream if stream is not None else None)
        if stream is not None:
            stream.synchronize()
        return d_out.cpu().numpy().view(STATS_COLS_DTYPE)

    stranded = tasks.copy()
    stranded["reserved"] = np.where(a_rc, STATS_A_RC, 0) | np.where(b_rc, STATS_B_RC, 0)
    host_s = eng.stats_columns_pairs(stranded, cig)
    host_f = eng.stats_columns_pairs(tasks, cig)
    assert host_s.tobytes() != host_f.tobytes()
    assert on_device(stranded, 1, torch.cuda.Stream(device=dev)).tobytes() == host_s.tobytes()
    assert on_device(tasks, 0, torch.cuda.Stream(device=dev)).tobytes() == host_f.tobytes()
    assert on_device(tasks, 1, None).tobytes() == host_f.tobytes()  # (forward tasks through the strand kernels)
    # any_rc == 0: the bits are not looked at
    assert on_device(stranded, 0, None).tobytes() == host_f.tobytes()
    eng.close()


# ---- 8. `stats generate` on resident chromosomes ----------------------------------------------------------------------------------------
def test_stats_generate_resident_writes_the_same_table(oracle, tmp_path):
    from sedef_amd import host
    from sedef_amd.build import build_library
    from test_stats_generate import _handmade, _stage
    build_library()
    host.build_host()
    # the hand-made input: hits on both strands whose alignments span runs of 100+ N
    fa, _, bed = _handmade(tmp_path, np.random.default_rng(79))
    rc_hits = sum(ln.split("\t")[9] == "-" for ln in open(bed).read().splitlines())
    plain, res = str(tmp_path / "plain.tsv"), str(tmp_path / "resident.tsv")
    a = host.stats_generate(fa, bed, plain, resident=False)
    b = host.stats_generate(fa, bed, res, resident=True)
    assert rc_hits >= 3 and a[2] > a[1]  # reverse-strand hits; more pieces than hits: hits were cut at assembly gaps
    assert a == b and a[0] >= 8
    assert open(res, "rb").read() == open(plain, "rb").read()
    assert sum(row.split("\t")[9] == "-" for row in open(res).read().splitlines()[1:]) >= 3
    # the stage's own output for a small genome with planted duplications
    fa, _, bed = _stage(host, oracle, tmp_path, seed=23)
    a = host.stats_generate(fa, bed, plain, resident=False)
    b = host.stats_generate(fa, bed, res, resident=True)
    assert a == b and a[0] >= 8
    assert open(res, "rb").read() == open(plain, "rb").read()
