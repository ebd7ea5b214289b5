"""Winnowed minimizers of ranges of the resident pool and the index over them (sdf_pool_minimizers, sdf_pool_minimizers_device,
sdf_pool_minimizer_index; sedef_amd/csrc/minimizers.hip).

Expected values: the reference's own lists (tests/golden/minimizers_kat.json.gz) and tests/minim_model.py, whose literal deque
loop and whose closed form are checked against each other and against the fixture in tests/test_minimizers_cpu.py.  Every
comparison is exact, record for record."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import pytest
import torch  # (at collection: before the library brings a HIP runtime of its own along)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import minim_model as M  # noqa: E402
from test_minimizers_cpu import load_fixture  # noqa: E402

pytestmark = pytest.mark.gpu

SDF_ERR_UNSUPPORTED, SDF_ERR_INVALID, SDF_ERR_OVERFLOW = -3, -4, -5
NONE = 1 << 31


def dtypes():
    from sedef_amd.extz2 import MINIM_RANGE_DTYPE, MINIMIZER_DTYPE
    return MINIM_RANGE_DTYPE, MINIMIZER_DTYPE


def records(rows, rng_index):
    """(hash, loc, status) rows as the library's records of range `rng_index`."""
    rows = np.asarray(rows, np.int64).reshape(-1, 3)
    out = np.zeros(len(rows), dtypes()[1])
    out["hash"], out["loc"], out["status"], out["range"] = rows[:, 0], rows[:, 1], rows[:, 2], rng_index
    return out


def canaries(n):
    return np.frombuffer(b"\xEE" * (16 * n), dtypes()[1]).copy()


def sequence_of(pool, off, ln, rc):
    s = bytes(pool[off:off + ln])
    return M.rev_comp(s) if rc else s


def expected(pool, rows, k, w, sl, literal=False):
    """rows: (off, len, rc).  Returns (first, records) by the closed form (literal: by the deque loop as written)."""
    first, recs = [0], []
    for i, (off, ln, rc) in enumerate(rows):
        s = sequence_of(pool, off, ln, rc)
        r = records(M.get_minimizers(s, k, w, sl) if literal else M.closed_form_np(s, k, w, sl), i)
        recs.append(r)
        first.append(first[-1] + len(r))
    return np.array(first, np.int64), np.concatenate(recs) if recs else np.zeros(0, dtypes()[1])


def ranges_of(rows):
    r = np.zeros(len(rows), dtypes()[0])
    for i, (off, ln, rc) in enumerate(rows):
        r[i] = (off, ln, 1 if rc else 0)
    return r


def run(eng, rows, k, w, sl):
    code, first, out, used = eng.pool_minimizers_raw(ranges_of(rows), k, w, sl)
    assert code == 0, eng.lib.sdf_last_error(eng.ctx).decode()
    assert used == int(first[-1]) == len(out)
    return first.astype(np.int64), out


def same(got, want):
    gf, gr = got
    wf, wr = want
    assert np.array_equal(gf, wf), (gf[:10], wf[:10])
    assert gr.tobytes() == wr.tobytes(), [(i, gr[i], wr[i]) for i in np.flatnonzero(gr != wr)[:5]]


def sorted_records(recs, first):
    """A call's records in the index's order: (status, hash, loc) inside every range."""
    out = recs.copy()
    for a, b in zip(first[:-1], first[1:]):
        part = recs[a:b]
        out[a:b] = part[np.lexsort((part["loc"], part["hash"], part["status"]))]
    return out


def index_of(recs, first):
    """(n_groups, threshold) per range, by Index::Index as transcribed."""
    ng, thr = [], []
    for a, b in zip(first[:-1], first[1:]):
        g, t, _ = M.index([(int(r["hash"]), int(r["loc"]), int(r["status"])) for r in recs[a:b]])
        ng.append(g)
        thr.append(t)
    return np.array(ng, np.uint32), np.array(thr, np.uint32)


def lay_out(rng, seqs, gap=True):
    """Sequences into one pool, each at an offset whose residue mod 16 is drawn (bytes of other letters between them)."""
    parts, offs, at = [], [], 0
    for s in seqs:
        pad = int(rng.integers(0, 17)) if gap else 0
        parts.append(np.frombuffer(b"acgtNRT-"[:8], np.uint8)[rng.integers(0, 8, pad)])
        at += pad
        offs.append(at)
        parts.append(np.frombuffer(s, np.uint8))
        at += len(s)
    parts.append(np.frombuffer(b"GATTACA", np.uint8))
    return np.concatenate(parts), offs


@pytest.fixture(scope="module")
def eng():
    import sedef_amd
    e = sedef_amd.Extz2Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def kat():
    return load_fixture()


@pytest.fixture(scope="module")
def block(eng):
    b = int(eng.lib.sdf_minimizer_block())
    assert b % 64 == 0 and b > 1000
    return b


def test_fixture_cases_byte_for_byte(eng, kat):
    """Every case of the fixture through both entry points, the cases of one (k, w, separate_lowercase) in one call.  A
    reversed case lies in the pool as the fixture has it and carries SDF_MINIM_RC; a forward case of nothing but ACGTacgtN is
    given a second time as the reverse complement of its reverse complement: rc(seq) in the pool, SDF_MINIM_RC."""
    rng = np.random.default_rng(1)
    groups = {}
    for c in kat["cases"]:
        groups.setdefault((c["k"], c["w"], c["sl"]), []).append(c)
    n_twice = 0
    for (k, w, sl), cases in sorted(groups.items()):
        seqs, want, strands = [], [], []
        for c in cases:
            s = c["seq"].encode()
            seqs.append(s)
            want.append(c)
            strands.append(bool(c["rc"]))
            if not c["rc"] and set(s) <= set(b"ACGTacgtN"):
                seqs.append(M.rev_comp(s))
                want.append(c)
                strands.append(True)
                n_twice += 1
        pool, offs = lay_out(rng, seqs)
        eng.pool_upload(pool.tobytes())
        rows = [(o, len(s), rc) for o, s, rc in zip(offs, seqs, strands)]
        exp_first = np.concatenate([[0], np.cumsum([len(c["minimizers"]) for c in want])]).astype(np.int64)
        exp = np.concatenate([records(c["minimizers"], i) for i, c in enumerate(want)])
        same(run(eng, rows, k, w, sl), (exp_first, exp))
        first, srt, n_groups, threshold = eng.pool_minimizer_index(ranges_of(rows), k, w, sl)
        exp_sorted = np.concatenate([records([(h, loc, st) for st, h, locs in c["groups"] for loc in locs], i) for i, c in enumerate(want)])
        same((first, srt), (exp_first, exp_sorted))
        assert n_groups.tolist() == [c["n_groups"] for c in want] and threshold.tolist() == [c["threshold"] for c in want]
    assert n_twice > 50


def test_long_cases_move_the_threshold(eng, kat):
    def digest(r):
        return hashlib.sha256(np.stack([r["hash"].astype(np.int64), r["loc"], r["status"]], 1).astype("<i4").tobytes()).hexdigest()
    moved = 0
    for c in kat["long_cases"]:
        s = c["seq"].encode()
        eng.pool_upload(b"ca" + s + b"t")
        rows = [(2, len(s), bool(c["rc"]))]
        first, recs = run(eng, rows, c["k"], c["w"], c["sl"])
        assert len(recs) == c["n_minimizers"] and digest(recs) == c["minimizers_sha256"], c["name"]
        f2, srt, n_groups, threshold = eng.pool_minimizer_index(ranges_of(rows), c["k"], c["w"], c["sl"])
        assert np.array_equal(f2, first) and digest(srt) == c["groups_sha256"], c["name"]
        assert (int(n_groups[0]), int(threshold[0])) == (c["n_groups"], c["threshold"]), c["name"]
        moved += c["threshold"] != NONE
    assert moved >= 2


def test_pool_edges_and_unaligned_offsets(eng):
    rng = np.random.default_rng(2)
    n = 4099  # (no multiple of 16)
    pool = np.frombuffer(b"ACGTacgtNnR", np.uint8)[rng.integers(0, 11, n)].copy()
    pool[0], pool[n - 1] = 0xC1, 0xE7  # ('A' | 0x80 at the first byte, 'g' | 0x80 at the last: characters are taken & 127)
    eng.pool_upload(pool.tobytes())
    ref = pool & 127
    rows = []
    for rc in (False, True):
        for o in range(16):
            for ln in (12, 27, 28, 29, 45, 300):
                rows += [(o, ln, rc), (n - ln - o, ln, rc)]
        rows += [(0, n, rc), (1, n - 1, rc), (0, n - 1, rc), (n, 0, rc), (n - 11, 11, rc)]
    for k, w, sl in ((12, 16, True), (15, 1, False), (1, 40, True)):
        same(run(eng, rows, k, w, sl), expected(ref, rows, k, w, sl))


def test_block_seams(eng, block):
    """Ranges of B - 1, B, B + 1 and 2 B + w starts, k = 1 so that a character IS its key (T 3 > G 2 > C 1 > A 0), and k = 12:
    a root whose look-back crosses the seam between two blocks, equal keys on both sides of it, and the first record -- the
    largest root <= w -- at w, before w and at 0."""
    B = block
    rng = np.random.default_rng(3)
    for k, w in ((1, 16), (1, 1), (1, 1000), (12, 16), (15, 33)):
        seqs = []
        for nk in (B - 1, B, B + 1, 2 * B + w):
            ln = nk + k - 1
            base = np.frombuffer(b"GT", np.uint8)[rng.integers(0, 2, ln)]
            # a C just before the seam and an equal one just behind it: both are roots, neither suppresses the other; the A
            # further on is a root only because its window reaches back over the seam and finds nothing smaller
            a = base.copy()
            if k == 1 and w > 1 and nk > B + w:
                a[B - 1] = a[B] = ord("C")
                a[B + w - 1] = ord("A")
            seqs.append(a.tobytes())
            # equal keys all along: every start >= w is a record, on both sides of every seam
            seqs.append(b"A" * ln)
            # lower case across the seam: the status changes inside a k-mer that straddles it
            b = base.copy()
            b[B - 5:B + 7] |= 0x20
            seqs.append(b.tobytes())
        # the first record: the least key of [0, w] lies at w, at w - 1 (w is larger), and all are equal (the LAST one: w)
        if k == 1:
            seqs += [b"T" * w + b"A" + b"T" * 40, b"T" * (w - 1) + b"AG" + b"T" * 40 if w > 1 else b"AG" + b"T" * 40, b"C" * (w + 30),
                     b"A" + b"T" * (w + 30)]
        pool, offs = lay_out(rng, seqs)
        eng.pool_upload(pool.tobytes())
        rows = [(o, len(s), rc) for rc in (False, True) for o, s in zip(offs, seqs)]
        want = expected(pool, rows, k, w, True)
        if k == 1:
            f, r = want
            n = len(seqs)
            assert [int(r["loc"][f[i]]) for i in range(n - 4, n)] == [w, max(w - 1, 0), w, 0]
            if w == 16:  # (the planted sequence of 2 B + w starts is the tenth)
                locs = set(r["loc"][f[9]:f[10]].tolist())
                assert {B - 1, B, B + w - 1} <= locs
        same(run(eng, rows, k, w, True), want)
        same(run(eng, rows, k, w, False), expected(pool, rows, k, w, False))


def test_mixed_strands_empty_ranges_and_a_thousand_small_ones(eng):
    rng = np.random.default_rng(4)
    n = 30000
    pool = np.frombuffer(b"ACGTacgtNnR", np.uint8)[rng.choice(11, n, p=[.2, .2, .2, .2, .04, .04, .04, .04, .015, .015, .01])].copy()
    eng.pool_upload(pool.tobytes())
    rows = []
    for i in range(1000):
        ln = int(rng.integers(0, 120))
        rows.append((int(rng.integers(0, n - ln)), ln, bool(rng.integers(0, 2))))
        if i % 97 == 0:
            rows += [(int(rng.integers(0, n)), 0, False), (0, 5000, True), (n, 0, True), (n - 3000, 3000, False)]
    same(run(eng, rows, 12, 16, True), expected(pool, rows, 12, 16, True))
    same(run(eng, rows, 5, 3, False), expected(pool, rows, 5, 3, False))
    fwd = [(o, ln, False) for o, ln, _ in rows]
    same(run(eng, fwd, 12, 16, True), expected(pool, fwd, 12, 16, True))  # (the kernels without the strand test)
    first, srt, n_groups, threshold = eng.pool_minimizer_index(ranges_of(rows), 12, 16, True)
    wf, wr = expected(pool, rows, 12, 16, True)
    same((first, srt), (wf, sorted_records(wr, wf)))
    ng, thr = index_of(wr, wf)
    assert np.array_equal(n_groups, ng) and np.array_equal(threshold, thr) and (thr == np.uint32(NONE)).all()


def test_overflow_protocol(eng):
    rng = np.random.default_rng(5)
    pool = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 5000)]
    eng.pool_upload(pool.tobytes())
    rows = [(0, 2000, False), (100, 0, False), (1500, 3500, True)]
    wf, wr = expected(pool, rows, 12, 16, True)
    need = len(wr)
    for index in (False, True):
        buf = canaries(need + 4)
        launches = eng.last_launches()
        res = eng.pool_minimizers_raw(ranges_of(rows), 12, 16, True, cap=need - 1, out=buf, index=index)
        assert res[0] == SDF_ERR_OVERFLOW and res[3] == need and np.array_equal(res[1].astype(np.int64), wf)
        assert buf.tobytes() == canaries(need + 4).tobytes()  # (nothing written, below cap or behind it)
        assert eng.last_launches() == launches + 5  # (the count's launches, not the records')
        res = eng.pool_minimizers_raw(ranges_of(rows), 12, 16, True, cap=need, out=buf, index=index)
        assert res[0] == 0 and res[3] == need
        assert buf[:need].tobytes() == (sorted_records(wr, wf) if index else wr).tobytes()
        assert buf[need:].tobytes() == canaries(4).tobytes()


def test_refusals_launch_nothing(eng):
    n = 4099
    eng.pool_upload(b"ACGT" * 1024 + b"ACG")
    RANGE, REC = dtypes()
    ok = (10, 100, 0)

    def call(rows, k=12, w=16, index=False, r_null=False, first_null=False, used_null=False, out_null=False, res_null=False):
        r = np.zeros(len(rows), RANGE)
        for i, row in enumerate(rows):
            r[i] = row
        first = np.full(len(rows) + 1, 77, np.uint64)
        out = canaries(256)
        used = C.c_size_t(12345)
        ng, thr = np.zeros(len(rows), np.uint32), np.zeros(len(rows), np.uint32)
        head = (eng.ctx, None if r_null else r.ctypes.data, len(rows), k, w, 1, None if first_null else first.ctypes.data,
                None if out_null else out.ctypes.data, 256, None if used_null else C.byref(used))
        launches = eng.last_launches()
        if index:
            code = eng.lib.sdf_pool_minimizer_index(*head, None if res_null else ng.ctypes.data, None if res_null else thr.ctypes.data)
        else:
            code = eng.lib.sdf_pool_minimizers(*head)
        if code != 0:
            assert eng.last_launches() == launches and (out["hash"] == 0xEEEEEEEE).all(), rows
            assert eng.lib.sdf_last_error(eng.ctx).decode() != ""
        return code

    for index in (False, True):
        for bad in ((-1, 4, 0), (0, -1, 0), (n - 5, 6, 0), (n + 1, 0, 0), (0, n + 1, 0), (1 << 40, 5, 1)):
            for rows in ([bad], [ok, bad], [bad, ok]):
                assert call(rows, index=index) == SDF_ERR_INVALID
        for flags in (2, 3, 0x100, -2147483648):
            assert call([ok, (10, 100, flags)], index=index) == SDF_ERR_UNSUPPORTED
        for w in (0, -1, -2147483648):
            assert call([ok], w=w, index=index) == SDF_ERR_INVALID
        for k in (0, -1, 16, 17, 32):
            assert call([ok], k=k, index=index) == SDF_ERR_UNSUPPORTED
        from sedef_amd.extz2 import MINIM_MAX_W
        assert call([ok], w=MINIM_MAX_W + 1, index=index) == SDF_ERR_UNSUPPORTED
        assert call([ok], w=MINIM_MAX_W, index=index) == 0
        assert call([ok], index=index, r_null=True) == SDF_ERR_INVALID
        assert call([ok], index=index, first_null=True) == SDF_ERR_INVALID
        assert call([ok], index=index, used_null=True) == SDF_ERR_INVALID
        assert call([ok], index=index, out_null=True) == SDF_ERR_INVALID
        # nothing to do: SDF_OK without a launch
        launches = eng.last_launches()
        assert call([], index=index, r_null=True, first_null=True, used_null=True, out_null=True, res_null=True) == 0
        assert eng.last_launches() == launches
    assert call([ok], index=True, res_null=True) == SDF_ERR_INVALID
    # the refused calls left the context usable, and a call that runs counts its launches
    launches = eng.last_launches()
    assert call([ok, (0, 300, 1)]) == 0 and eng.last_launches() == launches + 6


def test_device_form_equals_the_host_form(eng):
    rng = np.random.default_rng(6)
    n = 20000
    pool = np.frombuffer(b"ACGTacgtNn", np.uint8)[rng.integers(0, 10, n)]
    eng.pool_upload(pool.tobytes())
    rows = [(int(rng.integers(0, 9000)), int(rng.integers(0, 11000)), bool(rng.integers(0, 2))) for _ in range(40)]
    rows += [(0, n, True), (5, 0, False), (3, n - 3, False)]
    RANGE, REC = dtypes()
    for any_rc in (1, 0):
        use = rows if any_rc else [(o, ln, False) for o, ln, _ in rows]
        first, recs = run(eng, use, 12, 16, True)
        same((first, recs), expected(pool, use, 12, 16, True))
        d_ranges = torch.from_numpy(ranges_of(use).view(np.uint8).copy()).cuda()
        d_first = torch.zeros(len(use) + 1, dtype=torch.int64, device="cuda")
        d_out = torch.full(((len(recs) + 3) * 16,), 0xEE, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()  # (the tensors were filled on torch's stream)
        eng.pool_sync()
        used = eng.pool_minimizers_device(d_ranges.data_ptr(), len(use), any_rc, d_first.data_ptr(), d_out.data_ptr(), len(recs))
        assert used == len(recs) and np.array_equal(d_first.cpu().numpy(), first)
        got = d_out.cpu().numpy()
        assert got[:len(recs) * 16].tobytes() == recs.tobytes() and (got[len(recs) * 16:] == 0xEE).all()
        # a capacity that is short: the need is reported and nothing is written at or behind it
        d_out.fill_(0xEE)
        torch.cuda.synchronize()
        used = C.c_size_t(0)
        code = eng.lib.sdf_pool_minimizers_device(eng.ctx, d_ranges.data_ptr(), len(use), any_rc, 12, 16, 1, d_first.data_ptr(),
                                                  d_out.data_ptr(), len(recs) - 7, C.byref(used), None)
        assert code == SDF_ERR_OVERFLOW and used.value == len(recs)
        got = d_out.cpu().numpy()
        assert got[:(len(recs) - 7) * 16].tobytes() == recs[:-7].tobytes() and (got[(len(recs) - 7) * 16:] == 0xEE).all()
    # a range the host form refuses has no records here, and its neighbours have theirs
    bad = ranges_of([(100, 900, False), (n - 5, 900, False), (200, 700, True)])
    bad[2]["flags"] = 3
    d_ranges = torch.from_numpy(bad.view(np.uint8).copy()).cuda()
    d_first = torch.zeros(4, dtype=torch.int64, device="cuda")
    d_out = torch.zeros(200 * 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    used = eng.pool_minimizers_device(d_ranges.data_ptr(), 3, 1, d_first.data_ptr(), d_out.data_ptr(), 200)
    wf, wr = expected(pool, [(100, 900, False)], 12, 16, True)
    assert d_first.cpu().numpy().tolist() == [0, len(wr), len(wr), len(wr)] and used == len(wr)
    assert d_out.cpu().numpy()[:len(wr) * 16].tobytes() == wr.tobytes()


def test_on_a_shared_pool():
    import sedef_amd
    owner, view = sedef_amd.Extz2Engine(0), sedef_amd.Extz2Engine(0)
    try:
        rng = np.random.default_rng(7)
        pool = np.frombuffer(b"ACGTacgtNn", np.uint8)[rng.integers(0, 10, 9001)]
        owner.pool_upload(pool.tobytes())
        assert view.pool_share(owner) == len(pool)
        rows = [(0, 9001, False), (17, 4000, True), (9001, 0, False), (5000, 4001, True)]
        want = expected(pool, rows, 12, 16, True)
        same(run(view, rows, 12, 16, True), want)
        same(run(owner, rows, 12, 16, True), want)
        first, srt, n_groups, threshold = view.pool_minimizer_index(ranges_of(rows), 12, 16, True)
        same((first, srt), (want[0], sorted_records(want[1], want[0])))
        owner.close()  # (the caller's error: the view is left with an empty pool and says so)
        code = view.pool_minimizers_raw(ranges_of([(0, 1, False)]), 12, 16, True)[0]
        assert code == SDF_ERR_INVALID
    finally:
        view.close()
        owner.close()


def test_offsets_beyond_2_to_31():
    """The construction of tests/test_gpu_pool_share.py: a small record behind 34 x 64 MiB of others."""
    import sedef_amd
    from test_gpu_pool_share import _free_device_bytes, as_fasta, small_record
    from test_gpu_resident_strand import rev_table
    rng = np.random.default_rng(13)
    small = small_record(rng, rev_table(), 1000)
    big_n = 64 << 20
    a = sedef_amd.Extz2Engine(0)
    try:
        if _free_device_bytes(a) < (8 << 30):
            pytest.skip("less than 8 GiB of device memory free")
        big = np.frombuffer(b"ACGTacgtNn", np.uint8)[rng.integers(0, 10, 1 << 20)]
        big = np.tile(big, big_n >> 20)
        for k in range(34):
            assert a.pool_append_fasta(big, big_n, big_n, big_n, reset=(k == 0)) == k * big_n
            a.pool_sync()
        base = a.pool_append_fasta(*as_fasta(small, 60))
        n = len(small)
        assert base == 34 * big_n > (1 << 31)
        edge = np.concatenate([big[-2000:], big[:2000]])  # (2^31 is where the 33rd copy starts)
        rows = [(base, n, False), (base, n, True), (base + 17, n - 18, True), ((1 << 31) - 2000, 4000, False), ((1 << 31) - 2000, 4000, True)]
        local = np.concatenate([small, edge])
        local_rows = [(0, n, False), (0, n, True), (17, n - 18, True), (n, 4000, False), (n, 4000, True)]
        same(run(a, rows, 12, 16, True), expected(local, local_rows, 12, 16, True))
    finally:
        a.close()


def test_random_sequences_against_the_model(eng):
    """200 sequences of up to 50,000 characters, every one a range of its own on a drawn strand, in calls of one (k, w,
    separate_lowercase) each: the closed form for all of them, the deque loop as written for the short ones."""
    rng = np.random.default_rng(8)
    alphabets = (b"ACGT", b"ACGTacgtNn", b"AC", b"ACGTacgtNnRy", b"AAAAAAAC")
    settings = [(12, 16, True), (15, 1, False), (1, 5, True), (8, 100, True), (3, 33, False)]
    n_literal = 0
    for call, (k, w, sl) in enumerate(settings):
        seqs = []
        for i in range(40):
            ln = int(rng.integers(0, 50001)) if i % 4 else int(rng.integers(0, 3000))
            ab = np.frombuffer(alphabets[int(rng.integers(0, len(alphabets)))], np.uint8)
            s = ab[rng.integers(0, len(ab), ln)].copy()
            for _ in range(int(rng.integers(0, 4))):  # soft-masked stretches and assembly gaps
                at, run_len = int(rng.integers(0, ln + 1)), int(rng.integers(1, 400))
                if rng.random() < 0.5:
                    s[at:at + run_len] |= 0x20
                else:
                    s[at:at + run_len] = ord("N")
            seqs.append(s.tobytes())
        pool, offs = lay_out(rng, seqs)
        eng.pool_upload(pool.tobytes())
        rows = [(o, len(s), bool(rng.integers(0, 2))) for o, s in zip(offs, seqs)]
        got = run(eng, rows, k, w, sl)
        same(got, expected(pool, rows, k, w, sl))
        short = [i for i, s in enumerate(seqs) if len(s) < 3000]
        lit = expected(pool, [rows[i] for i in short], k, w, sl, literal=True)
        for j, i in enumerate(short):
            a, b = got[1][got[0][i]:got[0][i + 1]], lit[1][lit[0][j]:lit[0][j + 1]]
            assert all(np.array_equal(a[f], b[f]) for f in ("hash", "loc", "status")), (k, w, i)
        n_literal += len(short)
    assert n_literal >= 40
