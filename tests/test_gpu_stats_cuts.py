"""GPU: the cuts of `stats generate` on the resident pool (sdf_stats_cuts_pairs / sdf_stats_cuts_pairs_device;
stats_cuts.hip) -- whole-alignment matches, the cuts at runs of 100+ N, trim_back / trim_front of every piece -- and
`stats generate` with SDF_STATS_RESIDENT=1 SDF_STATS_CUTS_DEVICE=1.

No expected value comes from the code under test: the records are those of tests/cuts_model.py, which walks column strings
one column at a time like the host and is itself held against ColAln / _subhit / _split_alignment of
tests/test_stats_generate.py (here for every hand-made case, and in tests/test_stats_cuts_cpu.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch  # (at collection: before the library brings a HIP runtime of its own along)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cuts_model  # noqa: E402
from test_gpu_stats_resident import rev_table  # noqa: E402

pytestmark = pytest.mark.gpu

UNSUPPORTED, INVALID, OVERFLOW = -3, -4, -5
STRANDS = ((False, False), (True, False), (False, True), (True, True))
FIELDS = ("begin", "end", "t_begin", "t_end", "matches")


@pytest.fixture(scope="module")
def tab():
    return rev_table()


@pytest.fixture(scope="module")
def eng():
    import sedef_amd
    e = sedef_amd.Extz2Engine(0)
    yield e
    e.close()


COMP = np.arange(256, dtype=np.uint8)
for x, y in zip(b"ACGTacgt", b"TGCAtgca"):
    COMP[x] = y


def stored(s, rc):
    """The pool bytes of a side the alignment reads as `s` (ACGTN of either case)."""
    v = np.frombuffer(s, np.uint8)
    return COMP[v[::-1]] if rc else v


class Batch:
    """Alignments laid into one pool; what the alignment reads is taken back from the pool bytes through the host's table."""

    def __init__(self, tab):
        self.tab, self.chunks, self.at, self.specs = tab, [np.frombuffer(b"ACGTACGTAC", np.uint8)], 10, []

    def put(self, v):
        self.chunks.append(np.asarray(v, np.uint8))
        self.at += len(v)
        self.chunks.append(np.frombuffer(b"acgtNNrX-"[: 1 + len(self.specs) % 9], np.uint8))  # (odd offsets, bytes of every kind between)
        self.at += len(self.chunks[-1])
        return self.at - len(self.chunks[-1]) - len(v)

    def add(self, name, a_pool, b_pool, runs, a_rc, b_rc):
        self.specs.append((name, self.put(a_pool), len(a_pool), self.put(b_pool), len(b_pool), runs, a_rc, b_rc))

    def add_strings(self, name, a, b, runs, a_rc, b_rc):
        self.add(name, stored(a, a_rc), stored(b, b_rc), runs, a_rc, b_rc)

    def finish(self):
        from sedef_amd.extz2 import STATS_A_RC, STATS_B_RC, STATS_TASK_DTYPE
        self.pool = np.concatenate(self.chunks)
        tasks, cig = np.zeros(len(self.specs), STATS_TASK_DTYPE), []
        for k, (_, ao, al, bo, bl, runs, a_rc, b_rc) in enumerate(self.specs):
            tasks[k] = (ao, bo, al, bl, len(cig), len(runs), (STATS_A_RC if a_rc else 0) | (STATS_B_RC if b_rc else 0))
            cig += [(n << 4) | op for op, n in runs]
        self.tasks, self.cig = tasks, np.array(cig, np.uint32)
        return self

    def sides(self, k):
        _, ao, al, bo, bl, _, a_rc, b_rc = self.specs[k]
        a, b = self.pool[ao:ao + al], self.pool[bo:bo + bl]
        return (self.tab[a[::-1]] if a_rc else a).tobytes(), (self.tab[b[::-1]] if b_rc else b).tobytes()

    def expected(self, scores=cuts_model.DEFAULT, columns_too=False):
        out = []
        for k, s in enumerate(self.specs):
            a, b = self.sides(k)
            recs = cuts_model.records(a, b, s[5], scores)
            if columns_too:
                cuts_model.check_against_column_model(a, b, s[5], recs)
            out.append(recs)
        return out


def as_lists(first, pieces):
    assert (pieces["flags"] == 0).all() and not pieces["reserved"].any()
    return [[tuple(int(pieces[f][j]) for f in FIELDS) for j in range(int(first[i]), int(first[i + 1]))] for i in range(len(first) - 1)]


def compare(batch, got, exp):
    assert len(got) == len(exp)
    bad = [k for k in range(len(exp)) if got[k] != exp[k]]
    assert not bad, (len(bad), batch.specs[bad[0]][0], batch.specs[bad[0]][6:], got[bad[0]], exp[bad[0]])


@pytest.fixture(scope="module")
def handmade(tab, eng):
    """Every hand-made case on all four strand combinations, in one pool and one call; the expected records once."""
    cases = cuts_model.handmade(np.random.default_rng(5))
    batch = Batch(tab)
    for a_rc, b_rc in STRANDS:
        for name, a, b, runs in cases:
            batch.add_strings(name, a, b, runs, a_rc, b_rc)
    batch.finish()
    assert eng.pool_upload(batch.pool.tobytes()) == len(batch.pool)
    exp = batch.expected(columns_too=True)
    first, pieces = eng.stats_cuts_pairs(batch.tasks, batch.cig)
    return batch, exp, as_lists(first, pieces), len(cases)


def test_handmade_cases_on_all_strands(handmade):
    batch, exp, got, n = handmade
    compare(batch, got, exp)
    by = {(s[0], s[6], s[7]): r for s, r in zip(batch.specs, got)}
    for a_rc, b_rc in STRANDS:  # the cases do what they are there for, on the device's own records
        g = lambda name: by[(name, a_rc, b_rc)]  # noqa: E731
        assert len(g("a99")) == 1 and len(g("a100")) == 2 and g("a101")[1][0] == 251
        assert g("ab100")[0][:2] == (0, 150) and g("ba100")[0][:2] == (0, 130)
        assert len(g("run to the last column")) == 1 and g("run from column 0")[0][:2] == (120, 400)
        assert [r[:2] for r in g("overlapping runs")] == [(0, 60), (200, 400)]
        assert len(g("run broken by a gap")) == 1 and len(g("gap beside the run")) == 2
        assert g("piece starts inside a gap run")[1][:4] == (205, 415, 215, 415)
        assert g("marker quirk, 5 leading matches")[0] == (0, 25, 0, 0, 0) and g("marker not met")[0] == (0, 25, 15, 25, 10)
        assert g("piece of mismatches")[0] == (0, 20, 0, 0, 0)
        assert g("whole piece scores 0")[0] == (0, 9, 5, 9, 4) and g("two suffixes of one score")[0] == (0, 13, 0, 13, 8)
        assert len(g("1121 runs")) == 3 and len(g("64 runs before the run")) == 3


def test_no_event_matches_equal_the_columns_call(handmade, eng):
    batch, exp, got, n = handmade
    cols = eng.stats_columns_pairs(batch.tasks, batch.cig)
    whole = [k for k in range(len(got)) if len(got[k]) == 1 and got[k][0][0] == 0]
    assert len(whole) == 4 * 5  # (a99, b99, the run to the last column, the broken run, "no event")
    for k in whole:
        assert got[k][0] == (0, int(cols["span"][k]), 0, int(cols["span"][k]), int(cols["matches"][k])), batch.specs[k][0]


def test_strand_dependent_n(tab, eng):
    """R, '-' and a byte >= 128 inside an N run are N on a reversed side only; on a forward side they break the run."""
    rng = np.random.default_rng(8)
    batch = Batch(tab)
    for a_rc, b_rc in STRANDS:
        for odd in (ord("R"), ord("-"), 0x80, 0x90):
            _, a, b, runs = ("x",) + cuts_model.make(rng, [(0, 150), (2, 3), (0, 250)], n_a=[(160, 270)], n_b=[(20, 130)])
            ap, bp = stored(a, a_rc).copy(), stored(b, b_rc).copy()
            ia, ib = int(np.flatnonzero(ap == 78)[55]), int(np.flatnonzero(bp == 78)[40])
            ap[ia] = odd
            bp[ib] = odd
            batch.add("odd %#x" % odd, ap, bp, runs, a_rc, b_rc)
    batch.finish()
    eng.pool_upload(batch.pool.tobytes())
    exp = batch.expected(columns_too=False)
    first, pieces = eng.stats_cuts_pairs(batch.tasks, batch.cig)
    got = as_lists(first, pieces)
    compare(batch, got, exp)
    for s, r in zip(batch.specs, got):  # a forward side's run of 110 is broken into two short ones: no event of that side
        assert len(r) == 1 + int(s[6]) + int(s[7]), (s[0], s[6:], r)


def test_random_batch_and_other_scores(tab, eng):
    rng = np.random.default_rng(9)
    batch = Batch(tab)
    for k in range(300):
        runs, cols = [], 0
        while cols < 120 or (len(runs) < 3 and rng.random() < 0.7):
            op = 0 if not runs or runs[-1][0] != 0 else int(rng.integers(1, 3))
            n = int(rng.integers(20, 260)) if op == 0 else int(rng.integers(1, 12))
            runs.append((op, n))
            cols += n
        if runs[-1][0] != 0:
            runs.append((0, int(rng.integers(5, 60))))
            cols += runs[-1][1]
        plant = lambda: [(s, s + int(rng.integers(90, 111))) for s in rng.integers(0, max(cols - 100, 1), int(rng.integers(0, 3)))]  # noqa: E731
        n_a = [(s, min(e, cols)) for s, e in plant()]
        n_b = [(s, min(e, cols)) for s, e in plant()]
        name, (a, b, runs) = "r%d" % k, cuts_model.make(rng, runs, n_a=n_a, n_b=n_b, sub=float(rng.choice([0.02, 0.3, 0.7])))
        batch.add_strings(name, a, b, runs, bool(rng.integers(0, 2)), bool(rng.integers(0, 2)))
    batch.finish()
    eng.pool_upload(batch.pool.tobytes())
    cut = 0
    for scores in (cuts_model.DEFAULT, (1, -1, -2, -1), (3, 0, 0, -2), (63, -63, -32, -31)):
        exp = batch.expected(scores)
        first, pieces = eng.stats_cuts_pairs(batch.tasks, batch.cig, scores=scores)
        compare(batch, as_lists(first, pieces), exp)
        cut = sum(len(r) > 1 for r in exp)
    assert cut >= 30 and sum(len(r) == 1 and r[0][0] == 0 for r in exp) >= 60


def test_contract(handmade, eng):
    from sedef_amd.extz2 import STATS_PIECE_DTYPE, SdfError
    batch, exp, got, n = handmade
    tasks, cig = batch.tasks[:n], batch.cig  # (the forward quarter)
    P = len(batch.pool)
    eng.pool_upload(batch.pool.tobytes())
    rc, first, pieces, used = eng.stats_cuts_pairs_raw(tasks, cig)
    need = sum(len(r) for r in exp[:n])
    assert rc == 0 and used == need == int(first[n]) and as_lists(first, pieces) == exp[:n]
    # one short of the need: the code, the need, and nothing behind the capacity is touched
    buf = np.zeros(need, STATS_PIECE_DTYPE)
    buf.view(np.int32)[:] = 0x5A5A5A5A
    before = eng.last_launches()
    rc, first2, _, used = eng.stats_cuts_pairs_raw(tasks, cig, cap=need - 1, pieces=buf)
    assert rc == OVERFLOW and used == need and (first2 == first).all()
    assert (buf.view(np.int32)[8 * (need - 1):] == 0x5A5A5A5A).all()
    assert eng.last_launches() > before  # (the count ran)

    def refused(code, t, c=cig, scores=cuts_model.DEFAULT, text=None):
        before = eng.last_launches()
        rc, _, _, _ = eng.stats_cuts_pairs_raw(t, c, scores=scores)
        assert rc == code and eng.last_launches() == before and eng.pool_bytes() == P
        if text:
            assert text in eng.lib.sdf_last_error(eng.ctx).decode()

    t = tasks.copy()
    t["reserved"][3] = 0x4
    refused(UNSUPPORTED, t, text="unknown stats task flag")
    for side in "ab":
        t = tasks.copy()
        t[side + "_off"][2] = P - int(t[side + "_len"][2]) + 1
        refused(INVALID, t, text="outside the resident pool")
        t = tasks.copy()
        t[side + "_len"][0] = (1 << 24) + 1
        refused(UNSUPPORTED, t, text="16 Mb")
    t = tasks.copy()
    t["cigar_off"][n - 1] = len(cig) - int(t["n_cigar"][n - 1]) + 1
    refused(INVALID, t, text="CIGAR range")
    refused(UNSUPPORTED, tasks, scores=(64, -4, -40, -1))
    refused(UNSUPPORTED, tasks, scores=(5, -4, -40, -24))
    # n == 0
    before = eng.last_launches()
    rc, first0, p0, used = eng.stats_cuts_pairs_raw(tasks[:0], cig)
    assert rc == 0 and used == 0 and first0.tolist() == [0] and eng.last_launches() == before
    # a CIGAR that does not fit: the flag on that alignment's one record, after the launches; the others as they were
    t = tasks.copy()
    t["a_len"][5] -= 1
    rc, first3, pieces3, used = eng.stats_cuts_pairs_raw(t, cig)
    assert rc == INVALID and "alignment 5: the CIGAR does not fit" in eng.lib.sdf_last_error(eng.ctx).decode()
    j = int(first3[5])
    assert int(first3[6]) == j + 1 and int(pieces3["flags"][j]) == 1
    keep = np.ones(used, bool)
    keep[j] = False
    assert as_lists(np.array([0, keep.sum()]), pieces3[:used][keep])[0] == [r for k, rr in enumerate(exp[:n]) if k != 5 for r in rr]
    with pytest.raises(SdfError, match="rc=%d" % INVALID):
        eng.stats_cuts_pairs(t, cig)
    # the context serves a correct call afterwards
    assert as_lists(*eng.stats_cuts_pairs(tasks, cig)) == exp[:n]


def test_device_form_and_shared_pool(handmade, eng):
    import sedef_amd
    from sedef_amd.extz2 import STATS_PIECE_DTYPE
    batch, exp, got, n = handmade
    eng.pool_upload(batch.pool.tobytes())
    host_first, host_pieces = eng.stats_cuts_pairs(batch.tasks, batch.cig)
    need = len(host_pieces)
    dev = torch.device("cuda", 0)
    d_tasks = torch.from_numpy(batch.tasks.view(np.uint8).copy()).to(dev)
    d_cig = torch.from_numpy(batch.cig.view(np.int32).copy()).to(dev)

    def on_device(cap, stream):
        d_first = torch.full((len(batch.tasks) + 1,), -1, dtype=torch.int64, device=dev)
        d_out = torch.full(((need + 1) * 8,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        eng.pool_sync()
        used = eng.stats_cuts_pairs_device(d_tasks.data_ptr(), len(batch.tasks), 1, d_cig.data_ptr(), d_first.data_ptr(), d_out.data_ptr(),
                                           cap, stream=stream.cuda_stream if stream is not None else None)
        if stream is not None:
            stream.synchronize()
        return used, d_first.cpu().numpy(), d_out.cpu().numpy()

    used, first, out = on_device(need, None)
    assert used == need and (first == host_first).all() and (out[8 * need:] == 0x5A5A5A5A).all()
    assert out[:8 * need].view(STATS_PIECE_DTYPE).tobytes() == host_pieces.tobytes()
    used, first, out = on_device(need, torch.cuda.Stream(device=dev))
    assert (first == host_first).all() and out[:8 * need].view(STATS_PIECE_DTYPE).tobytes() == host_pieces.tobytes()
    # a capacity below the need on a stream of the caller's: first[n] says so, and no record lies at or past the capacity
    cap = need - 3
    _, first, out = on_device(cap, torch.cuda.Stream(device=dev))
    assert int(first[-1]) == need and (out[8 * cap:] == 0x5A5A5A5A).all()
    whole = int(np.searchsorted(host_first, cap, side="right")) - 1  # alignments whose pieces all lie below the capacity
    assert out[:8 * int(host_first[whole])].view(STATS_PIECE_DTYPE).tobytes() == host_pieces[:int(host_first[whole])].tobytes()
    # a view of the pool (sdf_pool_share) gives the same records
    view = sedef_amd.Extz2Engine(0)
    view.pool_share(eng)
    v_first, v_pieces = view.stats_cuts_pairs(batch.tasks, batch.cig)
    assert (v_first == host_first).all() and v_pieces.tobytes() == host_pieces.tobytes()
    view.close()
    assert as_lists(host_first, host_pieces) == exp


def test_cli_writes_the_same_table(tmp_path):
    from sedef_amd import host
    from sedef_amd.build import build_library
    from sedef_amd.host import CLI
    from test_stats_generate import _handmade
    build_library()
    host.build_host()
    fa, _, bed = _handmade(tmp_path, np.random.default_rng(79))

    def run(env, *args):
        e = {k: v for k, v in os.environ.items() if k not in ("SDF_STATS_RESIDENT", "SDF_STATS_CUTS_DEVICE")}
        e.update(env)
        r = subprocess.run([CLI, "stats", "generate"] + list(args) + [fa, bed], capture_output=True, text=True, env=e)
        assert r.returncode == 0, r.stderr
        return r

    both = {"SDF_STATS_RESIDENT": "1", "SDF_STATS_CUTS_DEVICE": "1"}
    plain, cuts = run({}), run(both)
    assert cuts.stdout == plain.stdout and plain.stdout.count("\n") >= 10 and "ignored" not in cuts.stderr
    gap = ("--max-ok-gap", "0", "--min-split", "200", "--uppercase", "10", "--max-error", "0.9")
    plain_gap, cuts_gap = run({}, *gap), run(both, *gap)
    assert cuts_gap.stdout == plain_gap.stdout and plain_gap.stdout != plain.stdout
    assert cuts_gap.stderr.count("SDF_STATS_CUTS_DEVICE=1 ignored") == 1
    # through the library too: the same table, and the same counts of hits, pieces and columns
    a = host.stats_generate(fa, bed, str(tmp_path / "a.tsv"))
    b = host.stats_generate_cuts(fa, bed, str(tmp_path / "b.tsv"))
    assert a == b and open(str(tmp_path / "a.tsv")).read() == open(str(tmp_path / "b.tsv")).read() == plain.stdout
