"""Ranges of the resident pool read back, by strand (sdf_pool_fetch_ranges / sdf_pool_fetch_ranges_device; seq_pack.hip:
pool_fetch_kernel).

The model is plain slicing for a forward range and tests/bruteforce.py: rc_model for a reversed one (rev_dna indexed c & 127:
case kept, everything that is not ACGTacgt becomes 'N'); every comparison is exact.  Destinations are laid out by the tests
themselves, with canaries around and between the ranges: no byte outside a range's destination may change."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu

SDF_ERR_UNSUPPORTED, SDF_ERR_INVALID = -3, -4
SEG = 16384  # SDF_FETCH_SEG_BYTES (include/sedef_hip.h): the destination bytes one group of sixteen lanes writes
POOL_LEN = 4099  # (deliberately no multiple of 16)
LENGTHS = (0, 1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257)
CANARY = 0xEE  # (no value rev_dna returns, and none the pools below hold where a canary is compared)
GUARD = 64


def rc_table():
    """rc_model (tests/bruteforce.py) per byte value, as a 256-entry table indexed by the whole byte: c & 127 first."""
    from bruteforce import rc_model
    tab = np.zeros(256, np.uint8)
    for c in range(256):
        tab[c] = ord(rc_model(chr(c & 127)))
    assert bytes(tab[list(b"ACGTacgtNnR-")]) == b"TGCAtgcaNNNN" and tab[0] == ord("N") and tab[0xC1] == ord("T")
    return tab


RC = rc_table()


def model(pool, off, ln, rc):
    a = pool[off:off + ln]
    return RC[a[::-1]] if rc else a


def make_pool(n=POOL_LEN, seed=7):
    rng = np.random.default_rng(seed)
    pool = np.frombuffer(b"ACGTacgtNn", np.uint8)[rng.integers(0, 10, n)].copy()
    planted = np.array(list(b"R-\0") + [0x80, 0x81, 0xC1, 0xE1, 0xC7, 0xF4, 0xFF, 0xCE], np.uint8)
    where = rng.choice(n, 6 * len(planted), replace=False)
    pool[where] = np.tile(planted, 6)
    pool[0], pool[n - 1] = 0xC1, 0xE7  # ('A' | 0x80 at the first byte, 'g' | 0x80 at the last)
    return pool


def fetch(eng, rows, dst_bytes, check=True):
    """rows: (off, len, rc, dst_off).  Returns the destination, GUARD canary bytes on either side of it included."""
    from sedef_amd.extz2 import POOL_FETCH_DTYPE
    r = np.zeros(len(rows), POOL_FETCH_DTYPE)
    for i, (off, ln, rc, d) in enumerate(rows):
        r[i] = (off, ln, 1 if rc else 0, d)
    buf = np.full(dst_bytes + 2 * GUARD, CANARY, np.uint8)
    rc = eng.lib.sdf_pool_fetch_ranges(eng.ctx, r.ctypes.data if len(r) else None, len(r), buf.ctypes.data + GUARD, dst_bytes)
    if check:
        assert rc == 0, eng.lib.sdf_last_error(eng.ctx).decode()
        return buf
    return rc, buf, eng.lib.sdf_last_error(eng.ctx).decode()


def expected(pool, rows, dst_bytes):
    exp = np.full(dst_bytes + 2 * GUARD, CANARY, np.uint8)
    for off, ln, rc, d in rows:
        exp[GUARD + d:GUARD + d + ln] = model(pool, off, ln, rc)
    return exp


def assert_same(got, exp, rows=None):
    bad = np.flatnonzero(got != exp)
    assert len(bad) == 0, (len(bad), [(int(i) - GUARD, int(got[i]), int(exp[i])) for i in bad[:8]])


def sweep_rows(rng, gaps):
    """Every length x source offset mod 16 x destination offset mod 16 x strand: 10,240 ranges.  gaps=False: back to back, the
    destination offsets mod 16 are what the lengths make them; gaps=True: every range starts at the wanted destination offset
    mod 16, so up to fifteen canary bytes lie between two ranges."""
    rows, d = [], 0
    for rc in (False, True):
        for ln in LENGTHS:
            for s in range(16):
                for dm in range(16):
                    off = 16 * int(rng.integers(0, 240)) + s  # (at most 3,839 + 257: inside the pool)
                    if gaps:
                        d += (dm - d) % 16
                    rows.append((off, ln, rc, d))
                    d += ln
    return rows, d


@pytest.fixture(scope="module")
def resident():
    import sedef_amd
    eng = sedef_amd.Extz2Engine(0)
    pool = make_pool()
    assert eng.pool_upload(pool.tobytes()) == POOL_LEN
    yield eng, pool
    eng.close()


@pytest.fixture(scope="module")
def sweep(resident):
    """The alignment sweep with gaps, its expected destination and what the host form returned: shared with the device form."""
    eng, pool = resident
    rows, size = sweep_rows(np.random.default_rng(1), gaps=True)
    return rows, size, expected(pool, rows, size), fetch(eng, rows, size)


def test_alignment_sweep_with_gaps(resident, sweep):
    eng, pool = resident
    rows, size, exp, got = sweep
    assert len(rows) == 2 * len(LENGTHS) * 256
    for s in range(16):  # every source offset mod 16 met every destination offset mod 16, on both strands
        for rc in (False, True):
            assert {d % 16 for off, ln, r, d in rows if off % 16 == s and r == rc and ln} == set(range(16))
    assert (exp[GUARD:GUARD + size] == CANARY).sum() > len(rows)  # (the gaps: more than a canary byte per range)
    assert_same(got, exp)


def test_alignment_sweep_back_to_back(resident):
    eng, pool = resident
    rows, size = sweep_rows(np.random.default_rng(2), gaps=False)
    exp = expected(pool, rows, size)
    assert (exp[GUARD:GUARD + size] != CANARY).all()
    assert_same(fetch(eng, rows, size), exp)
    # the same ranges, destinations in the opposite order (nothing follows its predecessor)
    rev_rows = rows[::-1]
    assert_same(fetch(eng, rev_rows, size), exp)


def test_pool_edges(resident):
    eng, pool = resident
    rows, d = [], 3
    for rc in (False, True):
        for ln in (1, 15, 16, 17):
            rows.append((0, ln, rc, d))
            d += ln + 5
            rows.append((POOL_LEN - ln, ln, rc, d))
            d += ln
    rows.append((0, POOL_LEN, True, d))
    d += POOL_LEN
    rows.append((0, POOL_LEN, False, d + 1))
    d += POOL_LEN + 1
    assert_same(fetch(eng, rows, d + 2), expected(pool, rows, d + 2))


def segment_rows(rng, n):
    long_len = (1 << 20) + 3
    assert long_len > SEG and long_len % SEG
    rows, d = [(5, long_len, False, 7)], 7 + long_len
    for k in range(1000):
        ln = 1 + int(rng.integers(0, 40))
        rows.append((int(rng.integers(0, n - ln)), ln, bool(rng.integers(0, 2)), d))
        d += ln
        if k == 500:
            rows.append((11, long_len, True, d))
            d += long_len
    for ln in (SEG, SEG, SEG - 1, SEG + 1):
        for rc in (False, True):
            rows.append((int(rng.integers(0, 1000)), ln, rc, d))
            d += ln + (3 if rc else 0)
    return rows, d


@pytest.fixture(scope="module")
def big_pool():
    return make_pool((1 << 20) + 3 + 90, seed=9)


@pytest.mark.parametrize("piece", [None, 65536], ids=["one piece", "pieces of 64 KiB"])
def test_segmenting(big_pool, piece):
    """One range of 2^20 + 3 bytes on either strand among 1,000 tiny ones, and ranges of one segment, one less and one more;
    then the same through a staging buffer of 64 KiB, which cuts the long ranges into seventeen pieces each."""
    import sedef_amd
    eng = sedef_amd.Extz2Engine(0, config=dict(SDF_FETCH_STAGE_BYTES=piece) if piece else None)
    try:
        eng.pool_upload(big_pool.tobytes())
        rows, size = segment_rows(np.random.default_rng(3), len(big_pool))
        assert_same(fetch(eng, rows, size), expected(big_pool, rows, size))
    finally:
        eng.close()


def test_high_bytes(resident):
    """A forward range returns bytes of 128 and more unchanged; a reversed one returns rev_dna(c & 127) -- the rule
    tests/test_gpu_stats_resident.py pins for the stats call."""
    import sedef_amd
    eng = sedef_amd.Extz2Engine(0)
    try:
        pool = np.arange(256, dtype=np.uint8).repeat(3)
        eng.pool_upload(pool.tobytes())
        n = len(pool)
        rows = [(0, n, False, 0), (0, n, True, n), (384, 384, True, 2 * n), (385, 383, False, 2 * n + 384)]
        got = fetch(eng, rows, 3 * n)
        assert_same(got, expected(pool, rows, 3 * n))
        body = got[GUARD:-GUARD]
        assert (body[:n] == pool).all() and (body[n:2 * n] < 128).all()
        assert bytes(body[n:2 * n][::-1][[3 * 0xC1, 3 * 0xE7, 3 * 0x80, 3 * 0xCE]]) == b"TcNN"  # 'A'|128, 'g'|128, 0|128, 'N'|128
    finally:
        eng.close()


def test_overlapping_and_repeated_sources(resident):
    eng, pool = resident
    rows, d = [], 0
    for k in range(50):
        for rc in (False, True):
            rows.append((1000, 333, rc, d))
            d += 333
    for k in range(40):  # overlapping: each starts a byte behind the one before
        rows.append((2000 + k, 100, k % 2 == 1, d))
        d += 100
    assert_same(fetch(eng, rows, d), expected(pool, rows, d))


def test_after_append_fasta():
    """Two records as a file has them: ranges across what were line ends are the record's bases."""
    import sedef_amd
    from bruteforce import rc_model
    rng = np.random.default_rng(5)
    eng = sedef_amd.Extz2Engine(0)
    try:
        bases, at = [], []
        for k, (n_bases, line) in enumerate(((1003, 60), (77, 7))):
            b = np.frombuffer(b"ACGTacgtNnR", np.uint8)[rng.integers(0, 11, n_bases)].tobytes()
            raw = b"\n".join(b[i:i + line] for i in range(0, n_bases, line)) + b"\n"
            at.append(eng.pool_append_fasta(raw, n_bases, line, line + 1, reset=(k == 0)))
            bases.append(b)
        assert at == [0, 1003] and eng.pool_bytes() == 1080
        ranges = [(0, 1003), (55, 10), (59, 2), (0, 61), (115, 130), (1003, 77), (1003 + 5, 4), (1003 + 6, 2), (990, 40), (1079, 1)]
        whole = b"".join(bases)
        fwd = eng.pool_fetch(ranges)
        rev = eng.pool_fetch(ranges, rc=True)
        mixed = eng.pool_fetch(ranges, rc=[i % 2 == 0 for i in range(len(ranges))])
        for i, (off, ln) in enumerate(ranges):
            want = whole[off:off + ln]
            assert fwd[i] == want and b"\n" not in fwd[i]
            assert rev[i] == rc_model(want.decode()).encode()
            assert mixed[i] == (rev[i] if i % 2 == 0 else fwd[i])
        out, offsets = eng.pool_fetch_raw(ranges, rc=False)
        assert out.dtype == np.uint8 and out.tobytes() == b"".join(fwd) and offsets[-1] == len(out)
    finally:
        eng.close()


def test_on_a_view_and_after_the_owner_is_gone():
    import sedef_amd
    owner, view = sedef_amd.Extz2Engine(0), sedef_amd.Extz2Engine(0)
    try:
        pool = make_pool(seed=21)
        owner.pool_upload(pool.tobytes())
        assert view.pool_share(owner) == POOL_LEN
        rows, size = sweep_rows(np.random.default_rng(4), gaps=True)
        rows = rows[::7]
        mine = fetch(owner, rows, size)
        assert_same(mine, expected(pool, rows, size))
        assert_same(fetch(view, rows, size), mine)
        owner.close()  # (the caller's error: the view is left with an empty pool and says so)
        assert view.pool_bytes() == 0
        rc, buf, err = fetch(view, [(0, 1, False, 0)], 16, check=False)
        assert rc == SDF_ERR_INVALID and "range 0" in err and (buf == CANARY).all()
        d_any = C.c_void_p(256)  # (never dereferenced: the call is refused for the empty pool)
        assert view.lib.sdf_pool_fetch_ranges_device(view.ctx, d_any, 1, 0, 1, d_any, None) == SDF_ERR_INVALID
    finally:
        view.close()
        owner.close()


def test_offsets_beyond_2_to_31():
    """The construction of tests/test_gpu_pool_share.py: the small record behind 34 x 64 MiB of others, fetched on both strands."""
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
        edge = np.concatenate([big[-8:], big[:8]])  # (2^31 is where the 33rd copy starts)
        rows = [(base, n, False, 0), (base, n, True, n), (base + 17, 1001, True, 2 * n), ((1 << 31) - 8, 16, False, 2 * n + 1001),
                ((1 << 31) - 8, 16, True, 2 * n + 1017), (base - 5, 10, True, 2 * n + 1033)]
        got = fetch(a, rows, 2 * n + 1043)[GUARD:-GUARD]
        assert (got[:n] == small).all() and (got[n:2 * n] == RC[small[::-1]]).all()
        assert (got[2 * n:2 * n + 1001] == RC[small[17:1018][::-1]]).all()
        assert (got[2 * n + 1001:2 * n + 1017] == edge).all() and (got[2 * n + 1017:2 * n + 1033] == RC[edge[::-1]]).all()
        assert (got[2 * n + 1033:] == RC[np.concatenate([big[-5:], small[:5]])[::-1]]).all()
    finally:
        a.close()


def test_contract(resident):
    eng, pool = resident
    ok = (10, 100, False, 0)
    size = 512

    def refused(rows, code, index, dst_bytes=size):
        launches = eng.last_launches()
        rc, buf, err = fetch(eng, rows, dst_bytes, check=False)
        assert rc == code and ("range %d:" % index) in err, (rows, rc, err)
        assert (buf == CANARY).all(), rows
        assert eng.last_launches() == launches

    for bad in ((-1, 4, False, 200), (0, -1, False, 200), (POOL_LEN - 5, 6, False, 200), (POOL_LEN + 1, 0, False, 200),
                (0, POOL_LEN + 1, False, 200), (1 << 40, 5, True, 200),     # the source
                (0, 4, False, -1), (0, 4, True, size - 3), (0, 0, False, size + 1)):  # the destination
        refused([bad], SDF_ERR_INVALID, 0)
        refused([ok, bad], SDF_ERR_INVALID, 1)
        refused([bad, ok], SDF_ERR_INVALID, 0)
    from sedef_amd.extz2 import POOL_FETCH_DTYPE
    for flags in (2, 3, 0x100, -2147483648):
        r = np.zeros(3, POOL_FETCH_DTYPE)
        r[0], r[1], r[2] = (10, 100, 1, 0), (10, 100, 0, 100), (10, 100, flags, 200)
        buf = np.full(size, CANARY, np.uint8)
        assert eng.lib.sdf_pool_fetch_ranges(eng.ctx, r.ctypes.data, 3, buf.ctypes.data, size) == SDF_ERR_UNSUPPORTED
        assert "range 2:" in eng.lib.sdf_last_error(eng.ctx).decode() and (buf == CANARY).all()
    # pointers missing
    buf = np.full(size, CANARY, np.uint8)
    assert eng.lib.sdf_pool_fetch_ranges(eng.ctx, None, 1, buf.ctypes.data, size) == SDF_ERR_INVALID and (buf == CANARY).all()
    r = np.zeros(2, POOL_FETCH_DTYPE)
    r[1] = (10, 100, 0, 0)
    assert eng.lib.sdf_pool_fetch_ranges(eng.ctx, r.ctypes.data, 2, None, size) == SDF_ERR_INVALID
    assert "range 1:" in eng.lib.sdf_last_error(eng.ctx).decode()
    # nothing to do: SDF_OK, nothing written
    assert eng.lib.sdf_pool_fetch_ranges(eng.ctx, None, 0, None, 0) == 0
    r = np.zeros(3, POOL_FETCH_DTYPE)
    r[0], r[1], r[2] = (0, 0, 0, 0), (POOL_LEN, 0, 1, size), (5, 0, 0, 17)
    assert eng.lib.sdf_pool_fetch_ranges(eng.ctx, r.ctypes.data, 3, None, size) == 0
    rc, buf, _ = fetch(eng, [(0, 0, False, 0), (POOL_LEN, 0, True, size)], size, check=False)
    assert rc == 0 and (buf == CANARY).all()
    # the refused calls left the context usable
    assert_same(fetch(eng, [ok], size), expected(pool, [ok], size))


def test_empty_pool_holds_no_range():
    import sedef_amd
    eng = sedef_amd.Extz2Engine(0)
    try:
        rc, buf, err = fetch(eng, [(0, 0, False, 0), (0, 1, False, 0)], 16, check=False)
        assert rc == SDF_ERR_INVALID and "range 1:" in err and (buf == CANARY).all()
        rc, buf, _ = fetch(eng, [(0, 0, True, 3)], 16, check=False)
        assert rc == 0 and (buf == CANARY).all()
    finally:
        eng.close()


def test_exports_and_python_forms(resident):
    eng, pool = resident
    for name in ("sdf_pool_fetch_ranges", "sdf_pool_fetch_ranges_device", "sdf_pool_fetch_plan"):
        assert hasattr(eng.lib, name), name
    got = eng.pool_fetch([(0, 5), (4090, 9), (7, 0)], rc=[False, True, True])
    assert got == [pool[:5].tobytes(), model(pool, 4090, 9, True).tobytes(), b""]
    assert eng.pool_fetch([]) == []


def _device_fetch(eng, rows, size, any_rc):
    """The device form on torch tensors: records from sdf_pool_fetch_plan, a canary-filled destination at an odd address."""
    import torch
    from sedef_amd.extz2 import POOL_FETCH_DTYPE
    r = np.zeros(len(rows), POOL_FETCH_DTYPE)
    for i, (off, ln, rc, d) in enumerate(rows):
        r[i] = (off, ln, 1 if rc else 0, d)
    rc, recs, plan_rc, n_seg, nbytes, _ = eng.pool_fetch_plan(r, dst_bytes=size)
    assert rc == 0 and nbytes == sum(ln for _, ln, _, _ in rows)
    d_recs = torch.from_numpy(recs.view(np.uint8).copy()).cuda()
    d_buf = torch.full((size + 2 * GUARD + 3,), CANARY, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # (the tensors were filled on torch's stream)
    eng.pool_sync()
    eng.pool_fetch_device(d_recs.data_ptr(), len(rows), plan_rc if any_rc is None else any_rc, n_seg,
                          d_buf.data_ptr() + 3 + GUARD)  # (the context's stream: the call returns when it has drained)
    out = d_buf.cpu().numpy()
    assert (out[:3] == CANARY).all()
    return out[3:], plan_rc


def test_device_form_equals_the_host_form(resident, sweep):
    eng, pool = resident
    rows, size, exp, host = sweep
    got, any_rc = _device_fetch(eng, rows, size, None)
    assert any_rc == 1
    assert_same(got, host)
    # forward-only input with any_rc = 0: plain slicing
    fwd = [(off, ln, False, d) for off, ln, _, d in rows]
    got, any_rc = _device_fetch(eng, fwd, size, 0)
    assert any_rc == 0
    exp_fwd = np.full(size + 2 * GUARD, CANARY, np.uint8)
    for off, ln, _, d in fwd:
        exp_fwd[GUARD + d:GUARD + d + ln] = pool[off:off + ln]
    assert_same(got, exp_fwd)


def test_round_trip_with_the_dp_calls():
    """64 pairs of ranges, the reference side reversed: sdf_extz2_batch_pairs with SDF_TASK_T_RC on the ranges gives the scores
    and CIGAR words of sdf_extz2_batch on the bytes fetched here (coded as align_dna codes them)."""
    import sedef_amd
    from sedef_amd.extz2 import TASK_DTYPE, WANT_CIGAR, WANT_SCORE
    from test_gpu_resident_strand import ALIGN, fasta_chars, rc_bytes, rev_table
    rng = np.random.default_rng(77)
    tab = rev_table()
    n, L = 64, 1 << 16
    pool = fasta_chars(rng, L)
    half = pool[:L // 2].copy()
    sub = rng.random(len(half)) < 0.05
    half[sub] = np.frombuffer(b"ACGTacgt", np.uint8)[rng.integers(0, 8, int(sub.sum()))]
    pool[L // 2:] = rc_bytes(tab, half)  # (the second half mirrors the first: reversed targets are related to their queries)
    t = np.zeros(n, TASK_DTYPE)
    t["qlen"] = rng.integers(1, 400, n)
    t["tlen"] = np.clip(t["qlen"] + rng.integers(-6, 7, n), 1, None)
    t["q_off"] = rng.integers(0, L // 2 - 400, n)
    t["t_off"] = np.minimum(L - t["q_off"] - t["qlen"] - rng.integers(0, 3, n), L - t["tlen"])
    t["w"], t["zdrop"] = -1, -1
    eng = sedef_amd.Extz2Engine(0)
    try:
        eng.pool_upload(pool.tobytes())
        want = WANT_CIGAR | WANT_SCORE
        res, cig = eng.align_batch_pairs(t, want=want, t_rc=True)
        ranges = np.stack([np.stack([t["q_off"], t["t_off"]], 1).ravel(), np.stack([t["qlen"], t["tlen"]], 1).ravel()], 1)
        out, offsets = eng.pool_fetch_raw(ranges, rc=np.tile([False, True], n))
        t2 = t.copy()
        t2["q_off"], t2["t_off"] = offsets[0:-1:2], offsets[1::2]
        res2, cig2 = eng.align_batch(t2, ALIGN[out], want=want)
        assert (res["score"] == res2["score"]).all() and (res["n_cigar"] == res2["n_cigar"]).all()
        assert (res["n_cigar"] > 0).all() and (res["matches"] >= 0.7 * t["qlen"]).mean() > 0.5
        for k in range(n):
            a = cig[int(res["cigar_off"][k]):int(res["cigar_off"][k]) + int(res["n_cigar"][k])]
            b = cig2[int(res2["cigar_off"][k]):int(res2["cigar_off"][k]) + int(res2["n_cigar"][k])]
            assert np.array_equal(a, b), k
    finally:
        eng.close()
